// The k-mer SPECTRUM of a token row: which windows count and the bucket each one increments.  Plain
// integer code for host and device alike: pg_spectrum.hip calls it with one window per lane, tests/capi_spectrum/
// spectrum_check.cpp compiles the same lines for the CPU and holds them against a naive counter.
//
// Tokens are 1..symbols; 0 is padding or an unknown letter and may stand anywhere.  For a row t[0..l) and a window
// length k, window i (0 <= i <= l - k) COUNTS iff none of its k tokens is 0 - the one rule that covers padding, rows
// shorter than k and unknown letters.  Its code is the window read as a number in base `symbols`,
//     code = sum_j (t[i + j] - 1) * symbols^(k - 1 - j)            < symbols^k <= 2^31,
// and it increments
//     exact  (dims == 0):                     bucket = code,                                      D = symbols^k <= 32768
//     hashed (dims = 2^e, 64 <= dims <= 32768): bucket = (((code + 1) * 2654435761) mod 2^32) >> (32 - e),   D = dims
// in 32-bit unsigned arithmetic (code + 1 <= 2^31 fits).  A token above `symbols` is the caller's error (the kernel raises
// its flag word); its window is skipped here, so no bucket outside 0..D-1 is ever produced.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_SP_FN __host__ __device__ __forceinline__
#else
#define PG_SP_FN static inline
#endif

#define PG_SP_MAX_L 2048          // positions per row: a count is at most 2048, which fp16 holds exactly
#define PG_SP_MAX_K 6
#define PG_SP_MAX_D 32768         // the widest profile: 64 KiB of 16-bit counts
#define PG_SP_MIN_DIMS 64
#define PG_SP_HASH_MUL 2654435761u

// The profile width D of (k, symbols, dims), or -1 for arguments outside the contract.
PG_SP_FN int pg_sp_dims(int k, int symbols, int dims) {
  if (k < 1 || k > PG_SP_MAX_K || symbols < 2 || symbols > 255) return -1;
  unsigned long long codes = 1;
  for (int j = 0; j < k; ++j) codes *= (unsigned long long)symbols;
  if (codes > (1ull << 31)) return -1;
  if (dims == 0) return codes <= PG_SP_MAX_D ? (int)codes : -1;
  if (dims < PG_SP_MIN_DIMS || dims > PG_SP_MAX_D || (dims & (dims - 1))) return -1;
  return dims;
}

// The hash shift of a width: 0 in exact mode, else 32 - log2(dims) (6..26).
PG_SP_FN int pg_sp_shift(int dims) {
  if (dims == 0) return 0;
  int e = 0;
  while ((1 << e) < dims) ++e;
  return 32 - e;
}

// Window t[0..k): false when it does not count, else true and its bucket.  `shift` from pg_sp_shift.
PG_SP_FN bool pg_sp_window(const unsigned char *t, int k, int symbols, int shift, uint32_t *bucket) {
  uint32_t code = 0;
  for (int j = 0; j < k; ++j) {
    const uint32_t v = t[j];
    if (v == 0u || v > (uint32_t)symbols) return false;
    code = code * (uint32_t)symbols + (v - 1u);
  }
  *bucket = shift ? ((code + 1u) * PG_SP_HASH_MUL) >> shift : code;
  return true;
}
