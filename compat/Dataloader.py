"""Import shim for drivers written against the reference's Dataloader.py: the preprocessed crops come from
uint8 NHWC shards decoded once offline (see neural_image_compression_amd/data.py) instead of per-item PIL."""
from neural_image_compression_amd.data import (ShardDataset, ShardLoader, shard_from_image_files,  # noqa: F401
                                               write_shard)
# images of any size: what a `transform` of random crops gives the reference's datasets (Dataloader.py:12,32)
from neural_image_compression_amd.data import (RaggedShardDataset, RandomCropLoader, load_image_u8,  # noqa: F401
                                               write_ragged_shard)
