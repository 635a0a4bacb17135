/* Host-side entropy coder of the MI355X hot path.  The reference has NO entropy
 * coder or bitstream (it only estimates bits, RateDistortionLoss.py:13-18); this is the
 * piece a deployment needs next to the device kernels, and the check that estimated bpp ~ coded bpp.
 *
 * A carry-propagating 32-bit range coder (byte-wise renormalisation, 16-bit frequencies) driven by
 * the cumulative tables the device builds (lic_factorized_cdf_tables / lic_gmm_cdf_tables in lic.h):
 * table t has S symbols and S+1 uint32 entries, cum[0] = 0 < cum[1] < ... < cum[S] = 65536.
 * Symbol n is the integer  idx[n] = value - window_lo  of its table; 0 < idx < S-1 is coded
 * directly, idx <= 0 / idx >= S-1 code the edge symbol followed by an Elias-gamma escape of the
 * excess in equiprobable bits, so any integer is representable.  Serial by nature: runs on the host
 * CPU, one stream per latent tensor (as the north star states).  Plain C ABI, no GPU dependency. */
#ifndef LIC_CODEC_H
#define LIC_CODEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum lic_codec_status {
  LIC_CODEC_OK = 0,
  LIC_CODEC_ERR_INVALID = -1,  /* null pointer, bad sizes, malformed table */
  LIC_CODEC_ERR_OVERFLOW = -2, /* output buffer too small */
  LIC_CODEC_ERR_CORRUPT = -3   /* bitstream ended early or decoded an impossible escape */
};

/* upper bound of the encoded size of n symbols (escapes included for |excess| < 2^31) */
size_t lic_rc_bound(int64_t n);

/* tables: [T][S+1]; table_of[n] selects the table of symbol n (NULL: table n, i.e. T == n).
 * idx[n]: value - window_lo.  Writes *nbytes <= cap bytes to out. */
int lic_rc_encode(const uint32_t* tables, const int32_t* table_of, int32_t S, const int32_t* idx, int64_t n,
                  uint8_t* out, size_t cap, size_t* nbytes);
/* inverse: idx_out[n] for the same tables */
int lic_rc_decode(const uint8_t* in, size_t nbytes, const uint32_t* tables, const int32_t* table_of, int32_t S,
                  int64_t n, int32_t* idx_out);

/* Streaming decoder: the tables of later symbols may depend on symbols already decoded (the
 * masked-conv context model, decoded wavefront by wavefront: codec.ContextCodec).  `in` must stay valid until
 * lic_rc_decoder_free. */
typedef struct lic_rc_decoder lic_rc_decoder;
lic_rc_decoder* lic_rc_decoder_new(const uint8_t* in, size_t nbytes);
int lic_rc_decoder_next(lic_rc_decoder* dec, const uint32_t* tables, const int32_t* table_of, int32_t S, int64_t n,
                        int32_t* idx_out);
void lic_rc_decoder_free(lic_rc_decoder* dec);

/* -sum log2(freq/65536) of the coded symbols (escape bits included): the ideal size of the stream
 * for these tables, to compare with 8 * nbytes */
double lic_rc_ideal_bits(const uint32_t* tables, const int32_t* table_of, int32_t S, const int32_t* idx,
                         int64_t n);

/* ------------------------------------------------------------------------------------------
 * "rANS-64": a second coder for the y streams whose decoder also runs on the device (lic_rans_decode_step in
 * lic.h); the range coder above stays the default and codes z.  The same tables, one per symbol ([n][S+1]).
 *   L = 64 interleaved states of 32 bits, each in [2^16, 2^32); 16-bit probabilities; renormalisation by 16-bit
 *   little-endian words, at most one per symbol per lane.  The n symbols are split into steps (step_len[nsteps],
 *   in symbols, summing to n: the wavefront steps of codec.ContextCodec); inside a step symbol k belongs to lane
 *   k % 64 and round k / 64, a step's last round may be partial, and rounds never straddle steps.
 *   Decoding a round, active lanes:  slot = x & 0xFFFF;  s: cum[s] <= slot < cum[s+1];
 *     x = (cum[s+1] - cum[s]) * (x >> 16) + slot - cum[s];  lanes with x < 2^16 take one word each,
 *     x = (x << 16) | word[ptr + rank]  with rank = number of such lanes with a smaller lane id;  ptr += count.
 *   Encoding is the exact mirror: steps, rounds and lanes last to first; if x >= freq << 16 emit x & 0xFFFF and
 *   x >>= 16; then x = ((x / freq) << 16) + x % freq + start; words go towards lower addresses; every state
 *   starts at 2^16.  Stream = 64 little-endian uint32 final states (lane 0 first) + the words in reading order.
 *   Escapes: idx <= 0 / idx >= S-1 code the edge symbol as above, but the excess (-idx or idx - (S-1)) goes into
 *   a separate list of uint32, in symbol order, 32 bits each (an in-stream escape would break the lock step).
 * lic_rans_decode returns LIC_CODEC_ERR_CORRUPT for a truncated stream, a word or escape cursor past the end,
 * trailing unused words or escapes, and final states other than 2^16.
 *
 * "rANS-64 x G" (G = 1..8; codec.rans_deal is the definition): one image's symbols dealt to G independent rANS-64
 *   streams so that G waves can code them.  The symbols keep their coding order and their rounds; round r of EVERY
 *   step belongs to sub-stream r % G.  Sub-stream g is an ordinary rANS-64 stream over the symbols dealt to it, in
 *   their original order, with step lengths step_len_g[t] = the symbols of step t in rounds = g (mod G): its own 64
 *   states, words and escape list.  A step with fewer rounds than G gives some sub-streams a zero-length step; an
 *   image with fewer rounds than G gives some no symbol at all (256 bytes of states).  G = 1 is rANS-64.  The
 *   functions below code one sub-stream at a time: the composition needs no symbol of its own.
 * ------------------------------------------------------------------------------------------ */
/* upper bound of the stream of n symbols in bytes (256 + 2 n); the escape list has at most n entries */
size_t lic_rans_bound(int64_t n);
int lic_rans_encode(const uint32_t* tables, int32_t S, const int32_t* idx, int64_t n, const int64_t* step_len,
                    int64_t nsteps, uint8_t* out, size_t cap, size_t* nbytes, uint32_t* esc_out, size_t esc_cap,
                    size_t* nesc);
int lic_rans_decode(const uint8_t* in, size_t nbytes, const uint32_t* esc, size_t nesc, const uint32_t* tables,
                    int32_t S, int64_t n, const int64_t* step_len, int64_t nsteps, int32_t* idx_out);
/* The same coder for symbols that SHARE tables, lic_rc_encode's convention: tables is [T][S+1] and table_of[i] in
 * [0, T) selects the table of symbol i (NULL: table i, T is not read -- lic_rans_encode / lic_rans_decode).  The
 * hyper-latent z of codec.ContextCodec(z_coder="rans") is such a stream: T = M tables, table_of[k] = k % M, one step
 * of all the image's symbols dealt to G sub-streams.  Everything lic_rans_encode / lic_rans_decode refuse, and a
 * table_of entry outside [0, T): LIC_CODEC_ERR_INVALID, before anything is indexed with it.  Any S >= 2. */
int lic_rans_encode_shared(const uint32_t* tables, const int32_t* table_of, int32_t T, int32_t S, const int32_t* idx,
                           int64_t n, const int64_t* step_len, int64_t nsteps, uint8_t* out, size_t cap,
                           size_t* nbytes, uint32_t* esc_out, size_t esc_cap, size_t* nesc);
int lic_rans_decode_shared(const uint8_t* in, size_t nbytes, const uint32_t* esc, size_t nesc, const uint32_t* tables,
                           const int32_t* table_of, int32_t T, int32_t S, int64_t n, const int64_t* step_len,
                           int64_t nsteps, int32_t* idx_out);
/* lic_rc_ideal_bits' definition with 32 bits per escape instead of the Elias-gamma length */
double lic_rans_ideal_bits(const uint32_t* tables, const int32_t* table_of, int32_t S, const int32_t* idx,
                           int64_t n);

int lic_codec_version(void);

#ifdef __cplusplus
}
#endif
#endif
