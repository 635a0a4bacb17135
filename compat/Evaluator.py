from neural_image_compression_amd.evaluator import CompressionEvaluator, VisionCompressionEvaluator  # noqa: F401
