/*
 * prograph_hip.h — C ABI of the MI355X (gfx950) graph-construction hot path.
 *
 * The reference (acmater/prograph) has no FFI: its plug-in contract is the Python
 * distance-function protocol `distance(X (N,D), Y (M,D), similarity=False) -> (M,N)`
 * (prograph/distance/hamming.py:8-39, README.md:48) plus the stock torch ops that
 * `Prograph.build_graph` (prograph/prograph.py:656-765) and `Prograph.indexing`
 * (prograph/prograph.py:254-343) run on `cuda:0`.  Each entry point below names the
 * reference call site(s) it replaces; INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch tensors are the
 *     storage container); the library never allocates or frees device memory and never
 *     synchronises.  The all-pairs calls (pg_eps_slots[_sym], pg_eps_fill_rows,
 *     pg_knn_hamming[_round]) take a caller-owned `workspace` of pg_workspace_bytes(nrows)
 *     bytes: launch-private device state (the pass counters of the engine's persistent waves,
 *     the data probe's counts and decision words, and - kNN calls of more than 65 536 rows,
 *     5.2 MB - the partial neighbour lists of rows swept in column pieces; one word per row for
 *     the rows a kNN launch finishes separately; from 65 536 rows on also the plan, the pass lists
 *     and the delivered keys of the symmetric kNN sweep of a self graph, 4 * 256 bytes per row and
 *     ~90 MB of lists at 200 000 rows - the size follows the row count alone, so every all-pairs
 *     call of that many rows asks for it, whether its launch can be symmetric or not),
 *     initialised by the call on `stream`; ONE workspace per launch in flight - a workspace
 *     may be reused once the launch that got it has completed, or by later launches on the
 *     same stream;
 *   - every launch goes to the caller-supplied `stream` (a hipStream_t passed as void*,
 *     NULL = the null stream) on the CURRENT HIP device of the calling thread; calls are
 *     re-entrant per stream and per device;
 *   - return value: 0 = ok, >0 = a hipError_t from the launch, <0 = PG_E_* below;
 *     `pg_last_error()` returns a thread-local human readable message;
 *   - no exceptions cross the boundary.  Process-wide state, all of it host side: the
 *     thread-local error string, the per-device cache of the compute-unit count and of the
 *     engine instances' occupancy, and the run-time binding of RCCL (pg_comm_*).
 *
 * Token storage: bit-sliced records in chunk-major order ("planes").  A sequence of L tokens
 * of `bits` bits each is G = ceil(L/32) groups of `bits` bit-plane dwords: dword p*G+g (plane
 * major) has bit j = bit p of token 32g+j (positions past L are 0).  The W = G*bits dwords of a record
 * are split into Q = ceil(W/4) 16-byte chunks (tail dwords zero); chunk q of sequence n lives
 * at byte offset (q*Npad + n)*16, Npad = pg_npad(N) (a multiple of 256, sequences past N are
 * zero).  A 64-lane wavefront that owns 64 consecutive sequences therefore reads one chunk per
 * lane as a single fully coalesced 1 KiB `global_load_dwordx4`, and the Hamming distance of
 * two records is B+1 VALU instructions per 32 tokens (xor, v_bitop3 x (B-1), v_bcnt).
 * Behind the Q chunk arrays the buffer carries the SIGNATURE SECTION (32 * Npad bytes): per sequence
 * the 54-bit filter signature (its plane-0 bits, 64 positions XOR-folded to 54) as FP4 (E2M1) elements -
 * 1.0 per set bit, then ten 1.0 bias slots (0 for padding sequences) - per 32 sequences one 1 KiB block in
 * v_mfma_f32_32x32x64_f8f6f4 fragment order: the column operand of the matrix-core
 * filter stage of the all-pairs engine (prograph_amd/csrc/pg_mm.h) - and behind it the FOLD SECTION
 * (32 * Npad bytes): two 16-byte arrays of Npad entries with the sequence's plane folds (plane p's G
 * dwords XOR-ed into one), planes 0..3 and 4..7 (unused planes zero) - the operands of the engine's
 * folded-exact bound on dense data.  pg_pack_planes writes all three parts.
 * Buffer size: pg_planes_bytes(N, L, bits) = (pg_nchunks(L, bits) * 16 + 64) * pg_npad(N) bytes.
 */
#ifndef PROGRAPH_HIP_H
#define PROGRAPH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PG_ABI_VERSION 3   /* 2: plane buffers carry the signature and fold sections; 3: caller-owned workspace */

/* library error codes (negative return values) */
#define PG_E_BADARG   (-1)   /* NULL pointer, negative size, k out of range ...        */
#define PG_E_TOOLONG  (-2)   /* L > PG_MAX_L (PG_MAX_L_5BIT with 5 bit planes)          */
#define PG_E_TOOMANY  (-3)   /* N > PG_MAX_N_KNN (24-bit column index in packed keys)   */
#define PG_E_NODEV    (-4)   /* no HIP device / wrong architecture                      */
#define PG_E_COMM     (-5)   /* RCCL missing or a collective failed (pg_last_error)     */

#define PG_MAX_L      128          /* tokens per sequence, 8 bit planes                  */
#define PG_MAX_L_5BIT 255          /* tokens per sequence, 5 bit planes (distance fits uint8) */
#define PG_MAX_N_KNN  16777216     /* 2^24                                               */
#define PG_MAX_K      63           /* k+1 sorted keys live in the 64 lanes of one VGPR   */
#define PG_LEV_MAX_BAND 8          /* banded Levenshtein keeps 2*8+1 diagonals in registers */

/* bit planes per token: fixed when a matrix is packed, passed to every call that reads it */
#define PG_BITS_5 5                /* every token <= 31 (20 amino acids + pad): 6 VALU ops / 32 tokens */
#define PG_BITS_8 8                /* any byte token 0..255:                    9 VALU ops / 32 tokens */

/* comparator codes for pg_eps_*: the reference's `comp` argument (operator.le default,
 * prograph/prograph.py:665) restricted to the five orderings                      */
#define PG_CMP_LE 0
#define PG_CMP_LT 1
#define PG_CMP_EQ 2
#define PG_CMP_GE 3
#define PG_CMP_GT 4
/* OR-ed into `cmp` of pg_f16_eps_*, pg_minkowski_eps_*, pg_cosine_eps_* and pg_euclidean_eps_* (no other entry takes it): keep the pairs
 * with d == 0 (similarities: s == 1) that those entries otherwise exclude - the rows of QUERIES, where a vector
 * equal to the query is a hit.  Without the flag the entries behave as before.                                   */
#define PG_CMP_KEEP_ZERO 0x10

int         pg_version(void);
const char *pg_last_error(void);
int         pg_device_info(int *cu_count, int *wave_size, char *arch, int arch_len);

/* Npad for N sequences (multiple of 256); groups of 32 positions; 16-byte chunks per record. */
int64_t     pg_npad(int64_t n);
int         pg_ngroups(int l);
int         pg_nchunks(int l, int bits);
/* bytes of a plane buffer for n sequences of l tokens: chunk arrays + signature section */
int64_t     pg_planes_bytes(int64_t n, int l, int bits);
/* bytes of the launch-private `workspace` of an all-pairs call over nrows rows (see Conventions) */
int64_t     pg_workspace_bytes(int64_t nrows);

/*
 * pg_pack_planes — row-major tokens -> plane layout.
 * Replaces the H->D staging `torch.as_tensor(self(representation), dtype=float16,
 * device="cuda:0")[idxs,:]` (prograph/prograph.py:726) and the zero right-padding of
 * `clean_input` (prograph/distance/utils.py:32-38).
 *   src        (n, l) row-major, leading dimension `ld` ELEMENTS, element size
 *              `elem_bytes` in {1,2,4,8} (uint8 / int16 / int32 / int64 tokens)
 *   rows       optional int64[n] gather list (the reference's `idxs`), NULL = identity
 *   bits       PG_BITS_5 or PG_BITS_8
 *   planes     out, pg_planes_bytes(n,l,bits) bytes, fully overwritten (padding zeroed)
 *   flags      out, uint32[1]: set to 1 when some token is outside 0..2^bits-1 (such tokens
 *              are truncated; the caller must not use the result)
 */
int pg_pack_planes(const void *src, int elem_bytes, int64_t n, int l, int64_t ld,
                   const int64_t *rows, int bits, void *planes, int64_t npad, uint32_t *flags,
                   void *stream);

/*
 * pg_pack_bytes — tokenise AND pack on the device.
 * Replaces `Prograph.tokenize` (prograph/prograph.py:454-474: one np.where pass per alphabet letter over the
 * fixed-width byte view of the sequence strings, table :127) together with the staging above: `src` is that byte
 * view, (n, width) uint8 row-major (numpy 'S<width>' storage: short sequences are NUL padded), `lut256` the
 * 256-entry letter table on the device (letter j of the alphabet -> j+1, everything else -> 0).
 *   tokens_out optional uint8 (n, width) row-major: the token matrix itself, for hosts that expose it
 *   flags      as in pg_pack_planes (set when a table entry does not fit `bits` planes)
 */
int pg_pack_bytes(const uint8_t *src, int64_t n, int width, int64_t ld, const int64_t *rows, const uint8_t *lut256,
                  int bits, void *planes, int64_t npad, uint8_t *tokens_out, uint32_t *flags, void *stream);

/*
 * pg_hamming_dense — all-pairs Hamming distance matrix.
 * Replaces `torch.sum(X != Y[:,None,:], axis=2)` (prograph/distance/hamming.py:34;
 * K2+K3 of SURVEY.md §2.2).  out[m*ldo + n] = #{j : Y[m,j] != X[n,j]}, (M,N) like the
 * reference.  out_elem_bytes in {1,2,4,8}: uint8 / fp16 / int32 / int64 (= the reference's dtype).
 * fp16 holds the integer itself (exact up to 2048 positions): a block in that form is the operand of
 * pg_f16_knn / pg_f16_eps_* below - graphs of sequences longer than one record of the fused engines.
 * accumulate != 0 adds to `out` instead of overwriting it: sequences longer than one record
 * (255 / 128 tokens) are handled as a sum over column segments packed separately.
 */
int pg_hamming_dense(const void *x_planes, int64_t n, int64_t x_npad,
                     const void *y_planes, int64_t m, int64_t y_npad,
                     int l, int bits, void *out, int out_elem_bytes, int64_t ldo,
                     int accumulate, void *stream);

/*
 * pg_eps_slots — the N^2 pass of the epsilon-neighbourhood graph.
 * Replaces the hot loop `distance(X,batch)` -> `comp(d,eps) & (d>0)` -> `torch.where`
 * -> gather of `build_graph` (prograph/prograph.py:731-739; K2..K7) for rows
 * [row0, row0+nrows) of `row_planes` against all `ncols` sequences of `col_planes`.
 * For every row the matching column indices are written into the row's slot (capacity `cap`)
 * in ascending order of their 32-column tile - within one tile in any order: a slot is an
 * intermediate, pg_eps_compact puts every entry in its place (an entry is at most 31 positions
 * from it) - and the exact number of matches into counts[] even when it exceeds `cap`
 * (pg_eps_compact recomputes such rows).
 *   cmp, eps   PG_CMP_* and the threshold; pairs with d == 0 are always excluded
 *   slot_idx   int32 [nrows*cap], slot_w uint8 [nrows*cap], counts uint32 [nrows]
 */
int pg_eps_slots(const void *row_planes, int64_t row_npad, int64_t row0, int64_t nrows,
                 const void *col_planes, int64_t col_npad, int64_t ncols,
                 int l, int bits, int cmp, double eps, int cap,
                 int32_t *slot_idx, uint8_t *slot_w, uint32_t *counts, void *workspace, void *stream);

/*
 * Square self-graph variant of pg_eps_slots / pg_eps_compact: rows [0,n) against the same n sequences.
 * Hamming and the five comparators are symmetric, so every unordered pair is evaluated ONCE (the
 * reference evaluates both orders, prograph/prograph.py:731-739): a match (i, j), i < j, is written to
 * the front of row i's slot in column order and to the back of row j's slot in arrival order
 * (counts_lo[j] is an atomic counter, zeroed by the call).  The total per row is
 * counts_up[i] + counts_lo[i]: the caller adds them, scans (pg_exclusive_scan) and calls
 * pg_eps_compact_sym, which emits each CSR row in ascending column order (rows that overflow `cap`,
 * or hold more than 512 entries from below, are recomputed exactly as in pg_eps_compact).  n < 2^27.
 * The result is identical to pg_eps_slots + pg_eps_compact on the same input.
 */
int pg_eps_slots_sym(const void *planes, int64_t npad, int64_t n, int l, int bits, int cmp, double eps, int cap,
                     int32_t *slot_idx, uint8_t *slot_w, uint32_t *counts_up, uint32_t *counts_lo, void *workspace,
                     void *stream);
int pg_eps_compact_sym(const void *planes, int64_t npad, int64_t n, int l, int bits, int cmp, double eps, int cap,
                       const int32_t *slot_idx, const uint8_t *slot_w, const uint32_t *counts_up,
                       const uint32_t *counts_lo, const int64_t *indptr, int32_t *indices, uint8_t *weights,
                       int leave_overflow, void *stream);

/*
 * pg_exclusive_scan — indptr[0..n] = exclusive prefix sum of counts[0..n) (int64).
 * Replaces the per-row split of `prod_neighbours` (prograph/prograph.py:646-654).
 * `scratch` must hold pg_scan_scratch_bytes(n) bytes.
 */
int64_t pg_scan_scratch_bytes(int64_t n);
int pg_exclusive_scan(const uint32_t *counts, int64_t n, int64_t *indptr, void *scratch,
                      void *stream);

/*
 * pg_eps_compact — slots -> CSR.  indices/weights must hold indptr[nrows] entries.
 * Output: indices int32 ascending per row (the order `torch.where` yields,
 * prograph/prograph.py:736), weights uint8 = the Hamming distance.
 * Rows whose count exceeded `cap`: leave_overflow = 0 recomputes each of them here (one wavefront per
 * row over all columns: fine for a handful of rows); leave_overflow = 1 skips them and the caller runs
 * pg_eps_fill_rows over the list of such rows (the engine again, exact and at engine speed however
 * many rows overflow - dense graphs).
 */
int pg_eps_compact(const void *row_planes, int64_t row_npad, int64_t row0, int64_t nrows,
                   const void *col_planes, int64_t col_npad, int64_t ncols,
                   int l, int bits, int cmp, double eps, int cap,
                   const int32_t *slot_idx, const uint8_t *slot_w, const uint32_t *counts,
                   const int64_t *indptr, int32_t *indices, uint8_t *weights, int leave_overflow, void *stream);

/*
 * pg_eps_fill_rows — the epsilon pass for a LIST of rows, written straight into the CSR.
 * row_list: int64[n_list] row numbers relative to row0 (ascending or not); for each the matches among
 * all ncols columns go, in ascending column order, to indices/weights at indptr[row] (indptr as for
 * pg_eps_compact: relative to row0; the counts that produced it are exact, so the segments fit).
 * scratch_counts: uint32[n_list] (receives the per-row counts again).
 */
int pg_eps_fill_rows(const void *row_planes, int64_t row_npad, int64_t row0, const int64_t *row_list, int64_t n_list,
                     const void *col_planes, int64_t col_npad, int64_t ncols, int l, int bits, int cmp, double eps,
                     const int64_t *indptr, int32_t *indices, uint8_t *weights, uint32_t *scratch_counts, void *workspace,
                     void *stream);

/*
 * pg_knn_hamming — k nearest neighbours under the canonical (distance, index) order.
 * Replaces `torch.sort(distance(X,batch),dim=1)` + `[:,1:k+1]` (prograph/prograph.py:
 * 758-762; K8,K9): for each row the k+1 smallest (d, column) pairs are kept, rank 0 is
 * dropped (not "self": prograph/prograph.py:761-763), ranks 1..k are written.
 * Ranks that do not exist (ncols < k+1) get idx = -1, dist = 255.
 *   idx_out int32 [nrows*k], dist_out uint8 [nrows*k];  1 <= k <= PG_MAX_K
 */
int pg_knn_hamming(const void *row_planes, int64_t row_npad, int64_t row0, int64_t nrows,
                   const void *col_planes, int64_t col_npad, int64_t ncols,
                   int l, int bits, int k, int32_t *idx_out, uint8_t *dist_out,
                   void *workspace, void *stream);

/*
 * pg_knn_sym_plan — the pass plan of the symmetric kNN sweep (host only: no device is touched).
 * A self graph (rows and columns the same n sequences) on the 64-row matrix-core instance evaluates every
 * unordered pair once: row block b (64 rows) sweeps the super-tiles (128 columns) from its own, b / 2, on,
 * cut into pieces that `slots` persistent waves fetch in the order given here.  Entry i of `out` (four int32:
 * row block, first super-tile, end super-tile, piece number within the block); at most max_passes entries
 * are written (out may be NULL); returns the number of passes.  piece > 0: pieces of that many super-tiles
 * (tests); piece = 0: the guided rule, pieces of at least piece_min super-tiles (0: the library's default).
 */
int64_t pg_knn_sym_plan(int64_t n, int64_t slots, int piece, int piece_min, int32_t *out, int64_t max_passes);
/*
 * pg_knn_sym_plan_device — the same plan as the device computes it for a launch (tests: it is compared with
 * pg_knn_sym_plan without a kNN launch).  plan_out: device memory for max_passes entries of four int32,
 * piece_start_out: device memory for (n + 63) / 64 + 1 uint32 - the first pass of every row block, then the
 * number of passes.  Returns the number of passes; a plan of more than max_passes is an error, nothing runs.
 */
int64_t pg_knn_sym_plan_device(int64_t n, int64_t slots, int piece, int piece_min, int32_t *plan_out,
                               uint32_t *piece_start_out, int64_t max_passes, void *stream);

/*
 * pg_knn_hamming_round — kNN beyond 63 neighbours, 63/64 ranks per all-pairs round.
 * Round 1 (first_round = 1): like pg_knn_hamming (rank 0 dropped, ranks 1..k, k <= 63) and in
 * addition last_keys[row] = packed key (distance << 24 | column) of the last rank written.
 * Later rounds (first_round = 0): only pairs whose key is greater than floor_keys[row] (= the
 * previous round's last_keys) are candidates; the k <= 64 smallest of them are written, i.e. the
 * next k ranks of the same canonical order.  idx_out / dist_out hold nrows*k entries per round.
 */
int pg_knn_hamming_round(const void *row_planes, int64_t row_npad, int64_t row0, int64_t nrows,
                         const void *col_planes, int64_t col_npad, int64_t ncols, int l, int bits,
                         int k, int first_round, const uint32_t *floor_keys, uint32_t *last_keys,
                         int32_t *idx_out, uint8_t *dist_out, void *workspace, void *stream);

/*
 * pg_query_knn_hamming — k nearest DATABASE sequences of every QUERY sequence, ranks 0..k-1 of
 * each query's (distance, column) order (a query equal to a database row has that row first;
 * ties go to the lower column).  Query and database planes are packed with the same width l and
 * the same bits; ndb < 2^24 (the column field of the key).  1 <= k <= 64 per call.  floor_keys:
 * NULL for the first round, else per query the last key of the previous round (last_keys of that
 * call): only keys greater than it are candidates, so rounds of 64 continue the same order up to
 * any k.  last_keys (nullable): per query the key (distance << 24 | column) of rank k-1.
 * Ranks that do not exist get idx = -1, dist = 255 (and last key 0xFFFFFFFF).
 *   idx_out int32 [nq*k], dist_out uint8 [nq*k]
 * The database is swept in column pieces (a handful of queries still fills the chip) whose
 * sorted lists a second kernel merges; workspace holds them: pass workspace_bytes >=
 * pg_query_workspace_bytes(nq, ndb, k) for the planned piece count.  A smaller workspace gives
 * fewer pieces (the same result, slower); 0 bytes means one piece.  No host synchronisation.
 */
int64_t pg_query_workspace_bytes(int64_t nq, int64_t ndb, int k);
int pg_query_knn_hamming(const void *q_planes, int64_t nq, int64_t q_npad, const void *db_planes, int64_t ndb,
                         int64_t db_npad, int l, int bits, int k, const uint32_t *floor_keys, uint32_t *last_keys,
                         int32_t *idx_out, uint8_t *dist_out, void *workspace, int64_t workspace_bytes, void *stream);

/*
 * pg_query_eps_count / _fill — the eps rows of QUERY sequences against a DATABASE: per query the database columns j
 * with comp(d(query, j), eps), in ascending j, as a CSR.  Pairs with d == 0 are KEPT (a query equal to a database
 * row finds that row), otherwise cmp and eps as in pg_eps_slots: the five PG_CMP_* codes, eps any finite number.
 * Planes as for pg_query_knn_hamming (the same width l and bits); ndb is bounded by the int32 indices only.
 * pg_query_knn_hamming's sweep and grid (query groups x column pieces, so that one query still fills the chip), but
 * every wave of a workgroup takes a contiguous run of column tiles: per query the columns fall into nseg = 4 x
 * pieces consecutive SEGMENTS.  pg_query_eps_segments(nq, ndb) is the planned nseg (0 for an empty operand); any
 * multiple of 4 up to 4 x ceil(ndb / 128) gives the same result.  Both calls must get the same nseg.
 *   pg_query_eps_count   seg_counts u32 [nq*nseg]: the matches of segment s of query q at [q*nseg + s]
 *   pg_exclusive_scan    over those nq*nseg counts -> seg_indptr int64 [nq*nseg + 1]; entry q*nseg is row q's
 *                        indptr, the last entry nnz (the one host sync of the path reads it)
 *   pg_query_eps_fill    the sweep again: indices int32 [nnz] and weights uint8 [nnz] (the distances), every match
 *                        at its segment's offset plus its rank in the segment.  No atomics, no sort, no overflow.
 */
int64_t pg_query_eps_segments(int64_t nq, int64_t ndb);
int pg_query_eps_count(const void *q_planes, int64_t nq, int64_t q_npad, const void *db_planes, int64_t ndb,
                       int64_t db_npad, int l, int bits, int cmp, double eps, int64_t nseg, uint32_t *seg_counts,
                       void *stream);
int pg_query_eps_fill(const void *q_planes, int64_t nq, int64_t q_npad, const void *db_planes, int64_t ndb,
                      int64_t db_npad, int l, int bits, int cmp, double eps, int64_t nseg, const int64_t *seg_indptr,
                      int32_t *indices, uint8_t *weights, void *stream);

/*
 * pg_index_flags — the fused 1xN pass of `Prograph.indexing` (prograph/prograph.py:
 * 298-325): distance of every sequence to reference row `ref`, a 256-bin histogram of
 * those distances (for the `d in np.unique(d_data)` assertion, :305), and
 * flags[n] = dist_ok(n) && pos_ok(n) where
 *   dist_ok = want_dist == NULL || bit d of the 256-bit set want_dist[8] is set
 *   pos_ok  = pos_mode == 0, or: (pos_mode 1 "or": some byte selected by pos_mask
 *             differs from the reference row; 2 "and": all selected bytes differ) and no
 *             byte selected by not_mask differs          (:316-325)
 * l: the number of positions of the packed rows, 1..255 with 5 bit planes, 1..128 with 8; anything beyond is refused.
 * pos_mask / not_mask: uint32[pg_ngroups(l)] device arrays, bit j of word g selects position 32g+j.
 *   dist_out uint8[n] (may be NULL), hist uint64[256] (may be NULL; must be zeroed by
 *   the caller), flags uint8[n] (may be NULL)
 */
int pg_index_flags(const void *planes, int64_t n, int64_t npad, int l, int bits,
                   int64_t ref, const uint32_t *want_dist, int pos_mode,
                   const uint32_t *pos_mask, const uint32_t *not_mask,
                   uint8_t *dist_out, uint64_t *hist, uint8_t *flags, void *stream);

/*
 * Banded Levenshtein kNN — BUILD DEFINED, no reference counterpart (BASELINE.json configs[4],
 * SURVEY.md §8 row a9; parity unpinned).  d(a,b) = min(edit_distance(a,b), band+1) over the
 * non-zero prefixes of zero-right-padded uint8 token rows (tokens 1..31); neighbours ordered by
 * (d, column), rank 0 dropped, ranks 1..k written (missing ranks: idx -1, dist 255).
 *   pg_lev_profile     tokens (n,l) row-major uint8 -> bag profiles (3*npad*16 bytes) + lens[n];
 *                      flags[0] = 1 if a token > 31 or an interior zero was seen
 *   pg_lev_candidates  all-pairs necessary-condition filter max(SAD, 2|dlen|) <= 2*band into
 *                      per-row candidate slots (ascending columns, exact counts[] even past cap;
 *                      the caller re-runs with a larger cap when max(counts) > cap)
 *   pg_lev_candidates_sym  the same for all rows at once with every unordered pair filtered once
 *                      (slots as in pg_eps_slots_sym: counts_up / counts_lo, the row itself in
 *                      neither); the caller re-runs with a larger cap when max(up + lo) > cap
 *   pg_lev_knn         exact banded edit distance per candidate (bit-parallel diagonal band) +
 *                      canonical kNN selection; `planes128` = the same tokens packed with
 *                      pg_pack_planes(bits = 5) at width l = 128 (chunk p = bit plane p);
 *                      counts_lo = NULL for pg_lev_candidates slots, else the symmetric pair.
 *                      slot_aux (int32 [n*cap], optional, filled by pg_lev_candidates_sym) holds for
 *                      every front entry the position of its mirror entry: with it and slot_w
 *                      (scratch, uint8 [n*cap]) every candidate PAIR is evaluated once and the
 *                      distance stored with both entries before the selection runs
 */
int pg_lev_profile(const uint8_t *tokens, int64_t n, int l, int64_t ld, void *profiles,
                   int64_t npad, int32_t *lens, uint32_t *flags, void *stream);
int pg_lev_candidates(const void *profiles, int64_t npad, int64_t n, int64_t row0, int64_t nrows,
                      int band, int cap, int32_t *slot_idx, uint8_t *slot_w, uint32_t *counts,
                      void *stream);
int pg_lev_candidates_sym(const void *profiles, int64_t npad, int64_t n, int band, int cap,
                          int32_t *slot_idx, uint8_t *slot_w, int32_t *slot_aux, uint32_t *counts_up,
                          uint32_t *counts_lo, void *stream);
int pg_lev_knn(const uint8_t *tokens, int64_t n, int l, int64_t ld, const void *planes128,
               int64_t npad, const int32_t *lens, int64_t row0, int64_t nrows, int band, int k,
               int cap, const int32_t *slot_idx, uint8_t *slot_w, const int32_t *slot_aux,
               const uint32_t *counts, const uint32_t *counts_lo, int32_t *idx_out, uint8_t *dist_out,
               void *stream);

/*
 * Exact Levenshtein distance — BUILD DEFINED like the banded kNN above, but without band or cap: unit cost
 * edit distance of the non-zero prefixes of zero-right-padded token rows (tokens 1..31, at most 128 positions;
 * what pg_lev_profile validates).  Operands are the rows packed with pg_pack_planes(bits = 5) at width
 * l = 128 (chunk p = bit plane p) plus their lengths (pg_lev_profile's lens).
 *   pg_levenshtein_dense  out[r * ldo + c] = d(Y row r, X row c) for all m x n pairs (Myers' bit-vector
 *                      recurrence on a 128-bit pattern, one X row per lane); out_elem_bytes 8 = int64,
 *                      2 = fp16 (distances are at most 128: exact), the block format of pg_f16_knn /
 *                      pg_f16_eps_*; l = width of the token rows (1..128), lengths are clamped to it.
 *                      A Y operand that starts at row r0 of a packed matrix is y_planes128 + 16 * r0 bytes,
 *                      y_lens + r0, with the matrix's npad.
 *   Epsilon graph of all rows (d > 0, comp(d, thr), comp = PG_CMP_LE / LT / EQ, thr in 0..8): after
 *   pg_lev_profile and pg_lev_candidates_sym with band >= thr (re-run with a larger cap while
 *   max(up + lo) > cap),
 *   pg_lev_eps_pairs   evaluates every candidate PAIR once - the banded distance min(d, band + 1), exact
 *                      where it is <= band - and stores it with both entries in slot_w;
 *   pg_lev_eps_count   counts_out[row] = number of kept entries; cmp | PG_CMP_KEEP_ZERO also keeps d = 0;
 *   pg_lev_eps_fill    after pg_exclusive_scan of those counts: int32 columns ascending within a row,
 *                      uint8 distances.  Same n, cap, cmp, thr and slots as the count.
 */
int pg_levenshtein_dense(const void *x_planes128, int64_t n, int64_t x_npad, const int32_t *x_lens,
                         const void *y_planes128, int64_t m, int64_t y_npad, const int32_t *y_lens, int l,
                         void *out, int out_elem_bytes, int64_t ldo, void *stream);
int pg_lev_eps_pairs(const uint8_t *tokens, int64_t n, int l, int64_t ld, const void *planes128,
                     int64_t npad, const int32_t *lens, int band, int cap, const int32_t *slot_idx,
                     uint8_t *slot_w, const int32_t *slot_aux, const uint32_t *counts_up,
                     const uint32_t *counts_lo, void *stream);
int pg_lev_eps_count(int64_t n, int cap, int cmp, int thr, const uint8_t *slot_w,
                     const uint32_t *counts_up, const uint32_t *counts_lo, uint32_t *counts_out,
                     void *stream);
int pg_lev_eps_fill(int64_t n, int cap, int cmp, int thr, const int32_t *slot_idx, const uint8_t *slot_w,
                    const uint32_t *counts_up, const uint32_t *counts_lo, const int64_t *indptr,
                    int32_t *indices, uint8_t *weights, void *stream);

/*
 * Exact Levenshtein distance beyond 128 positions — the definition above, unchanged, for operands of 1..PG_LEV_LONG_MAX_L
 * positions each (the two widths need not agree; PG_E_TOOLONG beyond): the block form of Myers' recurrence, one 128-bit
 * pattern block after the other per 128 text positions (prograph_amd/csrc/pg_lev_long.hip, pg_lev_long.h).
 *   pg_lev_long_pack   (n, l) row-major uint8 tokens, leading dimension ld, -> `planes`: ceil(l / 128) blocks x 5 bit
 *                      planes x npad uint4 (80 * ceil(l / 128) * npad bytes, npad = pg_npad(n)), uint4 number
 *                      (b * 5 + q) * npad + s = bit q of tokens 128 b .. 128 b + 127 of sequence s, so that block b of a
 *                      long operand is a short operand; `lens` int32 [n]; *flags (one word, zeroed on the stream first)
 *                      is set when a token is above 31 or a zero is not trailing padding.  No host sync.  The kernels
 *                      mask symbols and clamp lengths to the width: an invalid operand gives wrong numbers, never an
 *                      access out of bounds.
 *   pg_levenshtein_long_dense  out[r * ldo + c] = d(Y row r, X row c) for all m x n pairs, X packed at width xl, Y at
 *                      width yl; out_elem_bytes 8 = int64, 2 = fp16 (a distance is at most 2048, and fp16 holds every
 *                      integer up to 2048: exact), the block format of pg_f16_knn / pg_f16_eps_*.  A Y operand that
 *                      starts at row r0 of a packed matrix is y_planes + 16 * r0 bytes, y_lens + r0, with the matrix's
 *                      npad.  No workspace, no allocation; the kernel is instantiated for 1, 2, 4, 8 and 16 pattern
 *                      blocks and chosen by xl.
 * NULL pointers, non-positive sizes and a bad out_elem_bytes are PG_E_BADARG, checked before any launch.
 */
#define PG_LEV_LONG_MAX_L 2048
int pg_lev_long_pack(const uint8_t *tokens, int64_t n, int l, int64_t ld, void *planes, int64_t npad, int32_t *lens,
                     uint32_t *flags, void *stream);
int pg_levenshtein_long_dense(const void *x_planes, int64_t n, int64_t x_npad, const int32_t *x_lens, int xl,
                              const void *y_planes, int64_t m, int64_t y_npad, const int32_t *y_lens, int yl, void *out,
                              int out_elem_bytes, int64_t ldo, void *stream);

/*
 * Substitution-matrix distance — BUILD DEFINED (the reference has Hamming only, which is the table 1 - I):
 *     d(y, x) = sum_j C[y_j][x_j]     over zero-right-padded token rows, token 0 an ordinary index of C,
 * C symmetric with at most 32 symbols and entries 0..255 (the caller validates the table; the kernels mask tokens
 * to 0..31, so a bad operand gives wrong numbers, never an access out of bounds).
 *   pg_sub_pack        (n, l) row-major uint8 tokens, leading dimension ld, -> the transposed dword order the
 *                      dense kernel reads: dword g of sequence c (positions 4g..4g+3, low byte first) at byte
 *                      (g * npad + c) * 4, npad = pg_npad(n); positions past l and sequences past n are 0.
 *                      packed: ceil(l / 4) * npad * 4 bytes.  l <= 2048.  flags: uint32[1] the caller zeroes;
 *                      set to 1 when some token is >= a (1 <= a <= 32).  Positions [p, l) of a packed matrix,
 *                      p a multiple of 4, are the same buffer from byte (p / 4) * npad * 4 on.
 *   pg_substitution_dense  out[r * ldo + c] = d(Y row r, X row c) for all m x n pairs; both operands packed at
 *                      the same width l <= 2048 (PG_E_TOOLONG beyond).  cost_u8: the table as 32 x 32 bytes on
 *                      the device, rows and columns from the alphabet size on zero.  out_elem_bytes 8 = int64,
 *                      4 = int32, 2 = fp16 - the block format of pg_f16_knn / pg_f16_eps_*, exact while
 *                      d <= 2048, which the caller guarantees (l * max C <= 2048); the kernel does not test it.
 *                      accumulate != 0 adds to `out` instead of overwriting it, as in pg_hamming_dense: a
 *                      distance is the sum over column segments.  Sums are kept in 16-bit lanes for at most 120
 *                      positions (30 600 at cost 255) and widened when they are added into `out`, so any width
 *                      is exact in the integer outputs.  A Y operand that starts at row r0 of a packed matrix is
 *                      y_packed + 4 * r0 bytes with the matrix's npad.  Does not allocate; LDS only.
 */
int pg_sub_pack(const uint8_t *tokens, int64_t n, int l, int64_t ld, int a, void *packed, int64_t npad,
                uint32_t *flags, void *stream);
int pg_substitution_dense(const void *x_packed, int64_t n, int64_t x_npad, const void *y_packed, int64_t m,
                          int64_t y_npad, int l, const uint8_t *cost_u8, void *out, int64_t ldo,
                          int out_elem_bytes, int accumulate, void *stream);

/*
 * Gapped alignment distance - BUILD DEFINED (the reference has no such distance): global alignment (Needleman-Wunsch)
 * under a symmetric cost table C (at most 32 symbols, entries 0..255) with a linear gap penalty,
 *     H[0][j] = j * gap,  H[i][0] = i * gap,
 *     H[i][j] = min(H[i-1][j-1] + C[x_i][y_j], H[i-1][j] + gap, H[i][j-1] + gap),     d(y, x) = H[len x][len y],
 * a row's sequence being the row without its trailing zeros (an all-zero row is empty; an interior zero is symbol 0
 * of C).  With C = 1 - I and gap 1 it is the Levenshtein distance.
 *   pg_alignment_dense out[r * ldo + c] = d(Y row r, X row c) for all m x n pairs.  Both operands in the transposed
 *                      dword order of pg_sub_pack, X packed at width xl, Y at width yl, each <= 128 (PG_E_TOOLONG
 *                      beyond); the widths need not agree.  The lengths are found on the device, from the packed
 *                      tokens; tokens are masked to 0..31 (the caller validates them: pg_sub_pack's flags word).
 *                      cost_u8: the table as 32 x 32 bytes on the device (rows and columns from the alphabet size
 *                      on zero); gap in 1..255.  out_elem_bytes 8 = int64 (a distance is at most 128 * 255 = 32 640),
 *                      2 = fp16 - the block format of pg_f16_knn / pg_f16_eps_*, exact while d <= 2048, which the
 *                      caller guarantees (max(xl, yl) * max(max C, gap) <= 2048); the kernel does not test it.
 *                      A Y operand that starts at row r0 of a packed matrix is y_packed + 4 * r0 bytes with the
 *                      matrix's npad.  Does not allocate; LDS only.
 */
int pg_alignment_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                       int64_t y_npad, int yl, const uint8_t *cost_u8, int gap, void *out, int64_t ldo,
                       int out_elem_bytes, void *stream);

/*
 * The same distance with AFFINE gap penalties - BUILD DEFINED: a maximal run of g consecutive unaligned symbols of one
 * sequence costs gap_open + g * gap; a run in x directly followed by a run in y is two runs.  With e = gap, o = gap_open:
 *     H[0][0] = 0,  H[0][j] = o + j e,  H[i][0] = o + i e,
 *     E[i][j] = min(E[i-1][j] + e, H[i-1][j] + o + e),   F[i][j] = min(F[i][j-1] + e, H[i][j-1] + o + e),
 *     H[i][j] = min(H[i-1][j-1] + C[x_i][y_j], E[i][j], F[i][j]),                     d(y, x) = H[len x][len y]
 * (E[0][j] and F[i][0] infinite).
 *   pg_alignment_affine_dense  operands, cost table, lengths, output formats, row offsets and error codes as for
 *                      pg_alignment_dense; gap in 1..255, gap_open in 0..255 (PG_E_BADARG otherwise).  With
 *                      gap_open = 0 the result is pg_alignment_dense's.  A distance is at most
 *                      128 * 255 + 255 = 32 895; the fp16 output is exact while d <= 2048, which the caller
 *                      guarantees (max(xl, yl) * max(max C, gap) + gap_open <= 2048); the kernel does not test it.
 *                      Does not allocate; LDS only.
 */
int pg_alignment_affine_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                              int64_t y_npad, int yl, const uint8_t *cost_u8, int gap, int gap_open, void *out,
                              int64_t ldo, int out_elem_bytes, void *stream);

/*
 * LOCAL alignment score (Smith-Waterman, Gotoh's affine gaps) - BUILD DEFINED; a SIMILARITY: larger is nearer.  Under a
 * symmetric score table S (at most 32 symbols, entries -128..127), e = gap, o = gap_open:
 *     H[i][0] = H[0][j] = 0,  E[0][j] = F[i][0] = -inf,
 *     E[i][j] = max(E[i-1][j] - e, H[i-1][j] - o - e),   F[i][j] = max(F[i][j-1] - e, H[i][j-1] - o - e),
 *     H[i][j] = max(0, H[i-1][j-1] + S[x_i][y_j], E[i][j], F[i][j]),          s(y, x) = max over all i, j of H[i][j]:
 * the best score of any pair of substrings.  Sequences as for pg_alignment_dense (a row without its trailing zeros, an
 * interior zero is symbol 0 of S); padding never scores, whatever S[a][0] is.
 *   pg_alignment_local_dense  out[r * ldo + c] = s(Y row r, X row c).  Operands, lengths, output formats, row offsets,
 *                      checks and error codes as for pg_alignment_affine_dense; gap in 1..255, gap_open in 0..255
 *                      (0: linear gaps).  score_i8: the table as 32 x 32 signed bytes on the device (rows and columns
 *                      from the alphabet size on zero).  A score is at most min(len x, len y) * max(S) <= 128 * 127 =
 *                      16 256; the fp16 output is exact while s <= 2048, which the caller guarantees
 *                      (max(xl, yl) * max(S) <= 2048); the kernel does not test it.  Does not allocate; LDS only.
 */
int pg_alignment_local_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                             int64_t y_npad, int yl, const int8_t *score_i8, int gap, int gap_open, void *out,
                             int64_t ldo, int out_elem_bytes, void *stream);

/*
 * The two alignment recurrences above for sequences BEYOND 128 positions - BUILD DEFINED (pg_aln_long.hip): the Y side
 * is cut into strips of 128 positions, the strips' boundary columns pass through a caller-owned workspace.  Either
 * operand may have up to PG_ALN_LONG_MAX_L positions (PG_E_TOOLONG beyond); operands in the transposed dword order of
 * pg_sub_pack at their own widths, lengths found on the device, tokens masked to 0..31, as for pg_alignment_dense.
 *   pg_alignment_long_workspace  bytes of workspace for X operands of width xl: *one_workgroup_bytes = 256 * xl_padded * 4
 *                      (xl_padded = xl rounded up to 4), the least a call takes; *full_bytes = that times the workgroups
 *                      a whole device keeps in flight (compute units x resident workgroups).  Either pointer may be
 *                      NULL.  More workspace than full_bytes buys nothing.
 *   pg_alignment_long_dense  pg_alignment_affine_dense's arguments, results and error codes (gap_open = 0: the linear
 *                      penalty, exactly) with out_elem_bytes 4 = int32 (the block format of pg_i32_knn / pg_i32_eps_*)
 *                      or 8 = int64.  Launches at most workspace_bytes / one_workgroup_bytes workgroups, each looping
 *                      over its share of the (256 columns, 8 rows) tiles; a workspace smaller than one workgroup's
 *                      share is PG_E_BADARG.  The workspace may be handed to later work on the same stream.  Cells are
 *                      16 bits wide: the caller guarantees
 *                          max(xl, yl) * max(max C, gap) + 2 * gap_open + 2 * gap <= 65 535;
 *                      the kernel does not test it.
 *   pg_alignment_local_long_dense  the same for pg_alignment_local_dense's scores (score_i8 as there); the caller
 *                      guarantees min(xl, yl) * max(S) + 255 <= 65 535.
 */
#define PG_ALN_LONG_MAX_L 2048
int pg_alignment_long_workspace(int xl, int64_t *one_workgroup_bytes, int64_t *full_bytes);
int pg_alignment_long_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                            int64_t y_npad, int yl, const uint8_t *cost_u8, int gap, int gap_open, void *out,
                            int64_t ldo, int out_elem_bytes, void *workspace, int64_t workspace_bytes, void *stream);
int pg_alignment_local_long_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                                  int64_t y_npad, int yl, const int8_t *score_i8, int gap, int gap_open, void *out,
                                  int64_t ldo, int out_elem_bytes, void *workspace, int64_t workspace_bytes,
                                  void *stream);

/*
 * SEMI-GLOBAL ("overlap", end-gap-free) alignment score, Gotoh's affine gaps - BUILD DEFINED (pg_aln_semiglobal.hip); a
 * SIMILARITY: larger is nearer.  Both sequences are aligned end to end, the unaligned ends of either cost nothing.
 * Under a symmetric score table S (at most 32 symbols, entries -128..127), e = gap, o = gap_open:
 *     H[i][0] = H[0][j] = 0,  E[0][j] = F[i][0] = -inf,
 *     E[i][j] = max(E[i-1][j] - e, H[i-1][j] - o - e),   F[i][j] = max(F[i][j-1] - e, H[i][j-1] - o - e),
 *     H[i][j] = max(H[i-1][j-1] + S[x_i][y_j], E[i][j], F[i][j])                               (no zero floor),
 *     s(y, x) = max(max over i of H[i][len y], max over j of H[len x][j])                      (>= 0: H[0][len y] = 0).
 * Sequences as for pg_alignment_dense; padding never scores, whatever S[a][0] is.
 *   pg_alignment_semiglobal_dense  out[r * ldo + c] = s(Y row r, X row c).  Arguments, lengths, output formats (int64 /
 *                      fp16), row offsets, checks and error codes of pg_alignment_local_dense; at most 128 positions.
 *                      The fp16 output is exact while max(xl, yl) * max(S) <= 2048, which the caller guarantees.  Does
 *                      not allocate; LDS only.
 *   pg_alignment_semiglobal_long_dense  the same up to PG_ALN_LONG_MAX_L positions: the arguments, workspace
 *                      (pg_alignment_long_workspace), outputs (int32 / int64) and error codes of
 *                      pg_alignment_local_long_dense.  Cells are 16 bits wide and hold score + min(xl, yl) * max(S):
 *                      the caller guarantees 2 * min(xl, yl) * max(S) + 255 <= 65 535; the kernel does not test it.
 */
int pg_alignment_semiglobal_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                                  int64_t y_npad, int yl, const int8_t *score_i8, int gap, int gap_open, void *out,
                                  int64_t ldo, int out_elem_bytes, void *stream);
int pg_alignment_semiglobal_long_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                                       int64_t y_npad, int yl, const int8_t *score_i8, int gap, int gap_open, void *out,
                                       int64_t ldo, int out_elem_bytes, void *workspace, int64_t workspace_bytes,
                                       void *stream);

/*
 * FIT ("glocal") alignment score, Gotoh's affine gaps - BUILD DEFINED (pg_aln_fit.hip); a SIMILARITY: larger is nearer.
 * ALL of y is aligned, within ANY substring of x: only the ends of x are free.  Under a symmetric score table S (at most
 * 32 symbols, entries -128..127), e = gap, o = gap_open, i over x and j over y:
 *     H[i][0] = 0,  H[0][j] = -(o + j e) (j >= 1),  E[0][j] = F[i][0] = -inf,
 *     E[i][j] = max(E[i-1][j] - e, H[i-1][j] - o - e),   F[i][j] = max(F[i][j-1] - e, H[i][j-1] - o - e),
 *     H[i][j] = max(H[i-1][j-1] + S[x_i][y_j], E[i][j], F[i][j])                               (no zero floor),
 *     s(y, x) = max over i = 0..len x of H[i][len y].
 * NOT symmetric: the Y operand is the whole one.  -(o + e len y) <= s <= min(len x, len y) * max(0, max S): scores may be
 * NEGATIVE.  Sequences as for pg_alignment_dense; padding never scores, whatever S[a][0] is.
 *   pg_alignment_fit_dense  out[r * ldo + c] = s(Y row r, X row c) + bias.  Arguments, lengths, output formats (int64 /
 *                      fp16), row offsets, checks and error codes of pg_alignment_semiglobal_dense, and `bias` >= 0
 *                      (PG_E_BADARG below 0): a shift for callers whose next stage wants non-negative values; 0 gives
 *                      the scores.  At most 128 positions.  Cells are 16 bits wide and hold score + Z, Z = o + yl * (e +
 *                      max(0, max S)): the caller guarantees o + yl * (e + 2 max(0, max S)) + 255 <= 65 535 (128 positions
 *                      at 255 / 255 / 127 do not fit); the kernel does not test it.  The fp16 output is exact while every
 *                      out value is within 0..2048, which the caller guarantees.  Does not allocate; LDS only.
 *   pg_alignment_fit_long_dense  the same up to PG_ALN_LONG_MAX_L positions: the arguments, workspace
 *                      (pg_alignment_long_workspace), outputs (int32 / int64) and error codes of
 *                      pg_alignment_semiglobal_long_dense, `bias` and the caller's guarantee as above.
 */
int pg_alignment_fit_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                           int64_t y_npad, int yl, const int8_t *score_i8, int gap, int gap_open, int bias, void *out,
                           int64_t ldo, int out_elem_bytes, void *stream);
int pg_alignment_fit_long_dense(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                                int64_t y_npad, int yl, const int8_t *score_i8, int gap, int gap_open, int bias, void *out,
                                int64_t ldo, int out_elem_bytes, void *workspace, int64_t workspace_bytes, void *stream);

/*
 * PROFILE (PSSM) queries - BUILD DEFINED (pg_aln_profile.hip); SIMILARITIES: larger is nearer.  A profile is a table P of
 * L positions by A <= 32 symbols, entries -128..127; P[j][a] scores its position j against symbol a.  The recurrences are
 * those of pg_alignment_local_dense (mode 0), pg_alignment_semiglobal_dense (mode 1) and pg_alignment_fit_dense (mode 2)
 * with S[x_i][y_j] replaced by P[j][x_i]: the profile is the Y operand, all of its L positions count, and in mode 2 ALL of
 * it is placed within any stretch of the X row (scores may be negative).  No symmetry is asked of P.
 *   The operand.  profiles: bytes P[j][a] + bias, [m][32][lpad] with j contiguous, lpad a multiple of 128 that covers yl;
 *   bytes at j >= a profile's length and rows a >= A are 0.  lengths: int32[m] on the device, clamped to 0..yl by the
 *   kernels (nothing is found from bytes): an entry above yl counts yl positions, those behind the profile's own scoring
 *   -bias for every symbol (their bytes are 0); an entry of 0 or less is the empty profile, s = 0 in every mode (out_bias
 *   alone in mode 2).  yl: the longest length, which stands for the Y width in the modes' cell offsets.  bias = -min(0, min P) in 0..128 and top = max(0, max P) in 0..127 over the call's profiles: the caller
 *   computes them, there is no reduction on the device.  Row offsets: profiles + r0 * 32 * lpad, lengths + r0.
 *   pg_alignment_profile_dense  out[r * ldo + c] = s(profile r, X row c) + out_bias.  X as for pg_alignment_dense
 *                      (pg_sub_pack's order, x_npad a multiple of 256); xl, yl <= 128 (PG_E_TOOLONG beyond); gap in 1..255,
 *                      gap_open in 0..255; out_bias >= 0 is the shift of pg_alignment_fit_dense and is added in mode 2
 *                      alone; out_elem_bytes 8 (int64) or 2 (fp16).  mode outside 0..2, a bad lpad, bias or top:
 *                      PG_E_BADARG; the other checks and codes are pg_alignment_fit_dense's.  Every check returns before
 *                      any launch.  The caller guarantees the 16-bit cells with max P for max S - mode 0:
 *                      min(xl, yl) * top + 255 <= 65 535, mode 1: 2 * min(xl, yl) * top + 255 <= 65 535 (both always true
 *                      here), mode 2: gap_open + yl * (gap + 2 top) + 255 <= 65 535 - and, for the fp16 output, that every
 *                      out value is an integer within 0..2048; the kernel tests neither.  Does not allocate; LDS only.
 *   pg_alignment_profile_long_dense  the same up to PG_ALN_LONG_MAX_L positions on either side: the workspace of
 *                      pg_alignment_long_workspace(xl), out_elem_bytes 8 (int64) or 4 (int32), the checks and codes of
 *                      pg_alignment_fit_long_dense, the caller's guarantees as above.
 */
int pg_alignment_profile_dense(int mode, const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *profiles,
                               const int32_t *lengths, int64_t m, int lpad, int yl, int bias, int top, int gap, int gap_open,
                               int out_bias, void *out, int64_t ldo, int out_elem_bytes, void *stream);
int pg_alignment_profile_long_dense(int mode, const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *profiles,
                                    const int32_t *lengths, int64_t m, int lpad, int yl, int bias, int top, int gap,
                                    int gap_open, int out_bias, void *out, int64_t ldo, int out_elem_bytes, void *workspace,
                                    int64_t workspace_bytes, void *stream);

/*
 * Alignment TRACEBACK - BUILD DEFINED (pg_aln_trace.hip, pg_aln_trace.h): the canonical alignment of a list of pairs under
 * the tables H, E, F of pg_alignment_affine_dense (mode PG_ALN_TRACE_GLOBAL, table = cost_u8, gap_open = 0: the linear
 * form), pg_alignment_local_dense (PG_ALN_TRACE_LOCAL, table = score_i8) or pg_alignment_semiglobal_dense
 * (PG_ALN_TRACE_SEMIGLOBAL, score_i8); i runs over x, j over y, E leaves x_i unaligned, F leaves y_j unaligned.
 *   End cell: global (len x, len y); local the maximal H, ties to the smallest i, then the smallest j, a maximum of 0 the
 *   empty alignment at (0, 0); semi-global the best of H[i][len y] and H[len x][j], the same ties.
 *   Walk back from it in state H.  In H at (i, j): local stops where H[i][j] = 0, semi-global where i = 0 or j = 0, global
 *   at (0, 0) after leaving the j (i = 0) or i (j = 0) remaining symbols unaligned; otherwise a pair if
 *   H[i][j] = H[i-1][j-1] + T[x_i][y_j], else state E if H[i][j] = E[i][j], else state F, at the same cell.  In E: x_i
 *   unaligned, to (i-1, j), in state H if E[i][j] is the open term from H[i-1][j] (open wins a tie), else still in E.  F
 *   mirrors E along j.
 *   pg_alignment_trace_workspace  *bytes_per_wave = 64 * xl * ceil(yl / 8) * 4: the direction bits of 64 pairs.
 *   pg_alignment_trace  operands as for pg_alignment_dense (pg_sub_pack's order, widths xl, yl <= 128, PG_E_TOOLONG
 *                      beyond; x_npad >= n, y_npad >= m); xi, yi: int32[npairs] row numbers into the two operands, repeats
 *                      allowed; gap in 1..255, gap_open in 0..255.  head: int32 (npairs, 8) = score (the operator's value),
 *                      x_begin, x_end, y_begin, y_end (half-open ranges of the positions the alignment covers), n_ops,
 *                      identities (pairs with x_i = y_j), status.  ops: uint8 (npairs, ldo), ldo >= xl + yl: the columns
 *                      in forward order, 1 = pair, 2 = x symbol unaligned, 3 = y symbol unaligned, 0 from n_ops on (every
 *                      byte of a row is written: no zeroed buffer is needed).  A pair whose index lies outside its operand
 *                      touches no operand memory and gets status 1, n_ops -1, zeros elsewhere.  workspace: at least one
 *                      wave's share (PG_E_BADARG below it); the call launches min(ceil(npairs / 64), workspace_bytes /
 *                      share) waves, which stride over the list.  Every argument check returns before any launch.
 *   pg_alignment_trace_long_workspace, pg_alignment_trace_long (pg_aln_trace.hip)  the same canonical alignment,
 *                      arguments, outputs and checks for widths xl, yl of 1..2048 (PG_E_TOOLONG beyond; narrow operands
 *                      are accepted), the row of the tables cut into strips of 128 columns.  Cells are int32, so every
 *                      table and penalty of the three modes is exact: there is no "fits" condition.  *bytes_per_wave =
 *                      64 * xl * ceil(yl / 8) * 4 (direction bits) + 64 * xl * 8 (one boundary column between strips).
 *   pg_alignment_fit_trace, pg_alignment_fit_trace_long  the canonical alignment under pg_alignment_fit_dense's tables
 *                      (table = score_i8; x has the free ends, y is whole): the arguments, workspaces, outputs and checks
 *                      of the two entries above without `mode`, which go on rejecting every mode but 0, 1, 2.  End cell:
 *                      the best H[i][len y], i = 0..len x, ties to the smallest i ((0, len y) before any row).  The walk
 *                      stops in state H at j = 0; at i = 0 the j remaining symbols of y are left unaligned.  So y_begin = 0
 *                      and y_end = len y always, and x_begin:x_end is where y sits in x.
 */
#define PG_ALN_TRACE_GLOBAL 0
#define PG_ALN_TRACE_LOCAL 1
#define PG_ALN_TRACE_SEMIGLOBAL 2
int pg_alignment_trace_workspace(int xl, int yl, int64_t *bytes_per_wave);
int pg_alignment_trace(int mode, const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                       int64_t y_npad, int yl, const int32_t *xi, const int32_t *yi, int64_t npairs, const void *table, int gap,
                       int gap_open, int32_t *head, uint8_t *ops, int64_t ldo, void *workspace, int64_t workspace_bytes,
                       void *stream);
int pg_alignment_trace_long_workspace(int xl, int yl, int64_t *bytes_per_wave);
int pg_alignment_trace_long(int mode, const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                            int64_t y_npad, int yl, const int32_t *xi, const int32_t *yi, int64_t npairs, const void *table,
                            int gap, int gap_open, int32_t *head, uint8_t *ops, int64_t ldo, void *workspace,
                            int64_t workspace_bytes, void *stream);
int pg_alignment_fit_trace(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                           int64_t y_npad, int yl, const int32_t *xi, const int32_t *yi, int64_t npairs, const void *table,
                           int gap, int gap_open, int32_t *head, uint8_t *ops, int64_t ldo, void *workspace,
                           int64_t workspace_bytes, void *stream);
int pg_alignment_fit_trace_long(const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                                int64_t y_npad, int yl, const int32_t *xi, const int32_t *yi, int64_t npairs,
                                const void *table, int gap, int gap_open, int32_t *head, uint8_t *ops, int64_t ldo,
                                void *workspace, int64_t workspace_bytes, void *stream);

/*
 * Alignment STATISTICS - BUILD DEFINED (pg_aln_stats.hip, pg_aln_stats.h): the head of pg_alignment_trace without the
 * alignment's columns - what a percent-identity cut needs.  The canonical alignment is the one defined above, unchanged;
 * the forward recurrence hands every cell the counts of the predecessor the walk would choose, so no direction bits are
 * stored and nothing is walked back.
 *   pg_alignment_stats  mode 0, 1, 2 as above or 3 (fit: pg_alignment_fit_trace's alignment; table = score_i8, cost_u8
 *                      for mode 0); operands, xi, yi, gap and gap_open as for pg_alignment_trace (widths xl, yl of 1..128,
 *                      PG_E_TOOLONG beyond).  head: int32 (npairs, 8) = score, x_begin, x_end, y_begin, y_end, n_ops,
 *                      identities, status - equal, field for field, to the head pg_alignment_trace / pg_alignment_fit_trace
 *                      writes for the same pair.  There is no ops, no ldo and no workspace.  A pair whose index lies
 *                      outside its operand touches no operand memory and gets status 1, n_ops -1, zeros elsewhere.  At
 *                      most 1024 waves are launched; they stride over the list.  A bad mode, gap outside 1..255, gap_open
 *                      outside 0..255, NULL pointers, non-positive sizes and npad < n are PG_E_BADARG; every argument check
 *                      returns before any launch.
 */
int pg_alignment_stats(int mode, const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                       int64_t y_npad, int yl, const int32_t *xi, const int32_t *yi, int64_t npairs, const void *table, int gap,
                       int gap_open, int32_t *head, void *stream);

/*
 * Alignment values of an EDGE LIST - BUILD DEFINED (pg_aln_list.hip, pg_aln_list.h): the
 * value of every edge of a CSR list, on the row routines of the dense kernels - what rescoring a pool of candidate pairs
 * needs.
 *   pg_alignment_list_scores  mode 0 (global), 1 (local), 2 (semi-global) or 3 (fit), the numbering and the tables of
 *                      pg_alignment_stats (cost_u8 for mode 0, score_i8 otherwise); operands in pg_sub_pack's order at
 *                      widths xl, yl of 1..128 (PG_E_TOOLONG beyond); gap in 1..255, gap_open in 0..255.  indptr:
 *                      int64[m + 1], non-decreasing, indptr[0] = 0, one row per Y sequence; indices: int32[indptr[m]], X
 *                      column numbers.  scores[e], for e in indptr[r]..indptr[r + 1], is the value the dense entry of the
 *                      mode - pg_alignment_affine_dense (gap_open 0: the linear distance), _local_dense, _semiglobal_dense,
 *                      _fit_dense with bias 0 (true, possibly negative scores) - writes at out[r * ldo + indices[e]] with
 *                      out_elem_bytes 8.  An entry outside 0..n-1 (the -1 of an unfilled kNN slot) touches no operand
 *                      memory of its own and gets INT32_MIN.  Fit is exact while gap_open + yl * (gap + 2 * max S) + 255
 *                      <= 65 535, which the caller tests on the host as for pg_alignment_fit_dense.  One workgroup per 8
 *                      rows; a wave serves one row at a time, 64 entries a pass.  No workspace, no allocation.  A bad
 *                      mode, gap or gap_open, NULL pointers, non-positive sizes and npad < n are PG_E_BADARG; every
 *                      argument check returns before any launch.
 */
int pg_alignment_list_scores(int mode, const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, int64_t m,
                             int64_t y_npad, int yl, const int64_t *indptr, const int32_t *indices, const void *table, int gap,
                             int gap_open, int32_t *scores, void *stream);

/*
 * The same BEYOND 128 positions - BUILD DEFINED (pg_aln_list_long.hip, pg_aln_list_long.h): the strip
 * routines of the long dense kernels over the edge list.
 *   pg_alignment_list_long_scores  the arguments, the results and the errors of pg_alignment_list_scores, with two
 *                      differences: widths xl, yl of 1..2048 (PG_E_TOOLONG beyond), and a caller-owned workspace laid out
 *                      as the long dense entries' - a boundary column per lane of every workgroup in flight, shares sized
 *                      by pg_alignment_long_workspace(xl, &one, &full).  scores[e] is the value the LONG dense entry of
 *                      the mode - pg_alignment_long_dense, _local_long_dense, _semiglobal_long_dense, _fit_long_dense with
 *                      bias 0 - writes at out[r * ldo + indices[e]].  min(m, workspace_bytes / one) workgroups are
 *                      launched; they stride over the rows, and a row without a list costs two words of indptr.  A NULL
 *                      workspace, or one below a single share, is PG_E_BADARG.  The kernel does not test the 16-bit cell
 *                      bounds of the long dense entries (global: W * max(max C, gap) + 2 gap_open + 2 gap; local:
 *                      min(xl, yl) * max S + 255; semi-global: 2 * min(xl, yl) * max S + 255; fit: gap_open + yl * (gap +
 *                      2 * max S) + 255; each <= 65 535): the caller does.  Every argument check returns before any
 *                      launch; the entry never allocates.
 */
int pg_alignment_list_long_scores(int mode, const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed,
                                  int64_t m, int64_t y_npad, int yl, const int64_t *indptr, const int32_t *indices,
                                  const void *table, int gap, int gap_open, int32_t *scores, void *workspace,
                                  int64_t workspace_bytes, void *stream);

/*
 * k-mer SPECTRUM profiles - BUILD DEFINED (pg_spectrum.hip, pg_spectrum.h): the k-mer count vector of
 * every row of a token matrix, as the fp16 matrix pg_pack_f16 -> pg_cosine_prep -> pg_cosine_* / pg_euclidean_* take.
 * Tokens are 1..symbols; 0 is padding or an unknown letter and may stand anywhere.  Window i (0 <= i <= l - k) of a row
 * counts iff none of its k tokens is 0; code = sum_j (t[i+j] - 1) * symbols^(k-1-j).
 *   pg_spectrum_dims     the profile width D: symbols^k with dims == 0 (exact: bucket = code), dims itself otherwise
 *                        (hashed: bucket = (((code + 1) * 2654435761) mod 2^32) >> (32 - log2 dims)).  PG_E_BADARG for k
 *                        outside 1..6, symbols outside 2..255, symbols^k > 2^31, dims neither 0 nor a power of two in
 *                        64..32768, and dims == 0 with symbols^k > 32768.
 *   pg_spectrum_profile  tokens: (n, l) uint8, leading dimension ld, l <= 2048 (PG_E_TOOLONG beyond); rows: NULL, or n
 *                        int64 row numbers of `tokens` (output row r is token row rows[r]; the caller answers for their
 *                        range).  out_f16: fp16 row-major (n, D), leading dimension ldo >= D; exactly D elements of
 *                        every row are written, zeros included - a count is at most 2048 and exact in fp16.  flags: one
 *                        word, zeroed on the stream by this call and set when a token above `symbols` stands in the
 *                        rows read; such a window is skipped and nothing outside the row's D counts is touched.  The
 *                        arguments pg_spectrum_dims refuses, NULL tokens / out_f16 / flags, n <= 0, l <= 0, ld < l and
 *                        ldo < D are PG_E_BADARG; every check returns before any launch.  No workspace.
 */
int pg_spectrum_dims(int k, int symbols, int dims);
int pg_spectrum_profile(const uint8_t *tokens, int64_t n, int l, int64_t ld, const int64_t *rows, int k, int symbols, int dims,
                        void *out_f16, int64_t ldo, int32_t *flags, void *stream);

/*
 * pg_csr_row_stats — per-row reductions over a CSR graph for the analytics that consume the
 * `Neighbours` column (prograph/prograph.py:797-946: degree, laplacian, dirichlet, local_variance):
 *   deg[r] = sum_j w_rj,  sum_f[r] = sum_j f[col_j],  sum_wf[r] = sum_j w_rj * f[col_j],
 *   self_w[r] = weight of the entry whose column is the row's own node row0 + r (kNN lists of
 *   duplicated sequences contain it; the reference's Laplacian overwrites that diagonal term,
 *   prograph.py:894-896),  col_sum[c] += w_rc (in-degree, `mode="indegree"`; caller zeroes it).
 * weights: uint8 distances OR float32 (exactly one non-NULL; both NULL = boolean weights 1);
 * f = per-node values (double[ncols]); any output may be NULL.
 * An entry whose column is negative (the empty slot of a kNN table, idx = -1) is no edge: it adds to none of
 * deg, sum_f, sum_wf, self_w, col_sum, and neither f nor col_sum is read or written for it.  A column at or
 * past the length of f / col_sum is the caller's error and is not checked.
 */
int pg_csr_row_stats(const int64_t *indptr, const int32_t *indices, const uint8_t *weights_u8,
                     const float *weights_f32, int64_t nrows, int64_t row0, const double *f, double *deg,
                     double *sum_f, double *sum_wf, double *self_w, double *col_sum, void *stream);

/*
 * Undirected graphs from a device CSR (prograph_amd/csrc/pg_graph.hip, definitions in pg_graph.h): row sort, transpose,
 * symmetrisation.  G has nrows rows (indptr int64 [nrows + 1], indices int32 [nnz], weights of elem_bytes 1, 2 or 4), ncols
 * columns, and row r is node row0 + r.  An entry whose column is outside 0..ncols-1 is no edge (-1, the empty kNN slot, among
 * them): nothing is read through it or written for it.  Workspaces are the caller's (the *_workspace queries give their bytes,
 * 8-byte aligned; -1 for a negative size); the library allocates nothing.  NULL pointers, negative sizes, more than 2^31 - 1 rows
 * or columns, elem_bytes outside {1, 2, 4}, a bad kind / mode / combine and a workspace that is too small are PG_E_BADARG, checked
 * before any launch; nrows == 0 and nnz == 0 are legal and launch nothing that indexes.  A row of G holds fewer than 2^32 entries.
 *   pg_csr_sort_rows_count   counts[r] = the edges of row r; the workspace then holds the rows' keys (column << 32 | position in
 *                            row), sorted, no-edge entries last
 *   pg_csr_sort_rows_fill    after pg_exclusive_scan(counts) -> out_indptr: every row's edges ascending by column, equal columns
 *                            in storage order, weights moved with them bit for bit; same workspace, untouched in between
 *   pg_csr_histogram         counts[c] = the edges of column c (counts uint32 [ncols], zeroed here; integer atomics: exact)
 *   pg_csr_transpose         after pg_exclusive_scan(counts) -> t_indptr [ncols + 1]: row c of T lists (row0 + r, w) for every edge
 *                            (r, c, w) of G in G's storage order (columns of T ascending, duplicates in order); t_indices and
 *                            t_weights hold t_indptr[ncols] entries.  The same bits every run.  row0 + nrows <= 2^31 - 1.
 *   pg_csr_symmetrize_count  A = the sorted rows of a square G (row0 = 0, nrows = ncols), T = its transpose (nnz_a, nnz_t: the
 *                            lengths of their arrays, at least a_indptr[nrows], t_indptr[nrows]).  Merges A[r] and T[r] into
 *                            the workspace, combines the weights of every run of equal column - kind PG_W_UNSIGNED | PG_W_SIGNED
 *                            | PG_W_FLOAT (2 or 4 bytes), combine PG_COMBINE_MIN | PG_COMBINE_MAX; a NaN loses to a number,
 *                            ties (two NaNs, -0 and +0) go to the smaller bit pattern - and counts per row the columns that
 *                            mode keeps: PG_SYM_UNION all, PG_SYM_MUTUAL those that A[r] and T[r] both hold
 *   pg_csr_symmetrize_fill   after pg_exclusive_scan(counts) -> out_indptr: the kept columns ascending, each once, with the
 *                            combined weight; same nnz_a, nnz_t and workspace, untouched in between
 */
#define PG_W_UNSIGNED 0
#define PG_W_SIGNED 1
#define PG_W_FLOAT 2
#define PG_SYM_UNION 0
#define PG_SYM_MUTUAL 1
#define PG_COMBINE_MIN 0
#define PG_COMBINE_MAX 1
int64_t pg_csr_sort_workspace(int64_t nnz);
int pg_csr_sort_rows_count(const int64_t *indptr, const int32_t *indices, int64_t nrows, int64_t nnz, int64_t ncols,
                           uint32_t *counts, void *workspace, int64_t workspace_bytes, void *stream);
int pg_csr_sort_rows_fill(const int64_t *indptr, const void *weights, int elem_bytes, int64_t nrows, int64_t nnz,
                          const uint32_t *counts, const int64_t *out_indptr, int32_t *out_indices, void *out_weights,
                          const void *workspace, int64_t workspace_bytes, void *stream);
int pg_csr_histogram(const int32_t *indices, int64_t nnz, int64_t ncols, uint32_t *counts, void *stream);
int64_t pg_csr_transpose_workspace(int64_t nnz, int64_t ncols);
int pg_csr_transpose(const int64_t *indptr, const int32_t *indices, const void *weights, int elem_bytes, int64_t nrows,
                     int64_t nnz, int64_t ncols, int64_t row0, const int64_t *t_indptr, int32_t *t_indices, void *t_weights,
                     void *workspace, int64_t workspace_bytes, void *stream);
int64_t pg_csr_symmetrize_workspace(int64_t nnz_a, int64_t nnz_t);
int pg_csr_symmetrize_count(const int64_t *a_indptr, const int32_t *a_indices, const void *a_weights, int64_t nnz_a,
                            const int64_t *t_indptr, const int32_t *t_indices, const void *t_weights, int64_t nnz_t,
                            int elem_bytes, int kind, int mode, int combine, int64_t nrows, uint32_t *counts, void *workspace,
                            int64_t workspace_bytes, void *stream);
int pg_csr_symmetrize_fill(const int64_t *a_indptr, int64_t nnz_a, const int64_t *t_indptr, int64_t nnz_t, int elem_bytes,
                           int64_t nrows, const int64_t *out_indptr, int32_t *out_indices, void *out_weights,
                           const void *workspace, int64_t workspace_bytes, void *stream);

/*
 * pg_compact_flags — ascending indices of the non-zero flags (np.where(...)[0]).
 *   out_idx int64[n] (worst case), out_count int64[1]; scratch: pg_scan_scratch_bytes(n)
 */
int pg_compact_flags(const uint8_t *flags, int64_t n, int64_t *out_idx, int64_t *out_count,
                     void *scratch, void *stream);

/*
 * Minkowski (p = 2) graphs of fp16 embeddings: `build_graph(representation="Embedded",
 * distance=minkowski)`, prograph/distance/minkowski.py:8-41 through prograph/prograph.py:726-764.  Every
 * elementwise step rounds to fp16 exactly as the reference's fp16 tensor expression does (difference,
 * square, sum, root, and 1/(1+d) for similarities); see prograph_amd/csrc/pg_mink.hip for the tolerance.
 *   pg_pack_f16          (n, d) fp16 row-major (leading dimension ld elements, optional row gather list)
 *                        -> chunk-major: chunk q (8 halfs) of vector n at byte (q*npad + n)*16;
 *                        buffer pg_f16_nchunks(d) * npad * 16 bytes
 *   pg_minkowski_dense   out[m*ldo + n] = fp16 distance (similarity != 0: 1/(1+d)) of Y[m] and X[n]
 *   pg_f16_knn           ranks first..first+k-1 of every row of such a block in (value, column) order
 *                        (descending != 0: largest first, the similarity sort of :758); first + k <= 64
 *                        (more ranks: pg_f16_knn_round below)
 *   pg_f16_eps_count/_fill  comp(d, eps) & (d > 0)  [similarities: comp(eps, s) & (s < 1)], eps_f16 = the
 *                        threshold rounded to fp16 as torch does when it compares an fp16 tensor with a
 *                        Python number; count -> pg_exclusive_scan -> fill (columns ascending, fp16 weights)
 */
int pg_f16_nchunks(int d);
int pg_pack_f16(const void *src_f16, int64_t n, int d, int64_t ld, const int64_t *rows, void *packed, int64_t npad,
                void *stream);
int pg_minkowski_dense(const void *x_packed, int64_t n, int64_t x_npad, const void *y_packed, int64_t m,
                       int64_t y_npad, int d, int similarity, void *out_f16, int64_t ldo, void *stream);
int pg_f16_knn(const void *dist_f16, int64_t m, int64_t n, int64_t ld, int k, int first, int descending,
               int32_t *idx_out, void *w_out_f16, void *stream);
/*
 * pg_f16_knn_round — kNN beyond 63 neighbours on such a block, the pg_knn_hamming_round scheme: round 1 is pg_f16_knn
 * with first = 1, k = 63; every later round writes the next k (1..64) ranks of each row's (value, column) order,
 * i.e. the k smallest pairs strictly AFTER the row's floor: key > fk || (key == fk && column > fc).  The floor of row
 * r is the previous round's last output entry, read at floor_idx[r*floor_ld] / floor_w_f16[r*floor_ld] (its fp16
 * bits give the key back exactly, so no key array is needed; point both into the previous round's last column).
 * A floor index of -1 marks an exhausted row: the round writes idx -1, weight 0 for it, as for ranks that do not
 * exist.  Output rows are ldo elements apart (ldo >= k), so rounds write straight into column slices of one result.
 */
int pg_f16_knn_round(const void *dist_f16, int64_t m, int64_t n, int64_t ld, int k, int descending,
                     const int32_t *floor_idx, const void *floor_w_f16, int64_t floor_ld, int32_t *idx_out,
                     void *w_out_f16, int64_t ldo, void *stream);
int pg_f16_eps_count(const void *dist_f16, int64_t m, int64_t n, int64_t ld, int cmp, float eps_f16, int similarity,
                     uint32_t *counts, void *stream);
int pg_f16_eps_fill(const void *dist_f16, int64_t m, int64_t n, int64_t ld, int cmp, float eps_f16, int similarity,
                    const int64_t *indptr, int32_t *indices, void *weights_f16, void *stream);

/*
 * The same selection on (m, n) blocks of non-negative int32 values (leading dimension ld elements) - what
 * pg_alignment_long_dense writes with out_elem_bytes 4 (pg_select_i32.hip).  The stable (value, column) order of the fp16
 * entries, descending != 0: largest value first; int32 weights.
 *   pg_i32_knn           ranks first..first+k-1 of every row, first + k <= 64; a rank that does not exist: index -1,
 *                        weight 0
 *   pg_i32_knn_round     the floor scheme of pg_f16_knn_round: the next k (1..64) ranks strictly after each row's
 *                        floor - the previous round's last index and weight, read with row stride floor_ld - written
 *                        with row stride ldo
 *   pg_i32_eps_count/_fill  comp(v, thr) & (v > 0), cmp one of PG_CMP_*, thr an integer; cmp | PG_CMP_KEEP_ZERO:
 *                        comp(v, thr) & (v >= 0); count -> pg_exclusive_scan -> fill (columns ascending)
 */
int pg_i32_knn(const int32_t *vals, int64_t m, int64_t n, int64_t ld, int k, int first, int descending, int32_t *idx_out,
               int32_t *w_out, void *stream);
int pg_i32_knn_round(const int32_t *vals, int64_t m, int64_t n, int64_t ld, int k, int descending,
                     const int32_t *floor_idx, const int32_t *floor_w, int64_t floor_ld, int32_t *idx_out, int32_t *w_out,
                     int64_t ldo, void *stream);
int pg_i32_eps_count(const int32_t *vals, int64_t m, int64_t n, int64_t ld, int cmp, int64_t thr, uint32_t *counts,
                     void *stream);
int pg_i32_eps_fill(const int32_t *vals, int64_t m, int64_t n, int64_t ld, int cmp, int64_t thr, const int64_t *indptr,
                    int32_t *indices, int32_t *weights, void *stream);

/*
 * Fused Minkowski graphs: the distances of pg_minkowski_dense (same per-pair arithmetic, bit for bit) selected
 * on the fly in LDS tiles, so the (M, N) block never reaches HBM.  Replaces `distance(X, batch)` followed by
 * `torch.sort(...)[:, 1:k+1]` (prograph/prograph.py:726, :756-763) and by `comp(d, eps) & (d > 0)` ->
 * `torch.where` (:731-739) of `build_graph(representation="Embedded", distance=minkowski)`.  Operands as for
 * pg_minkowski_dense (pg_pack_f16 buffers; x_npad a multiple of 256, y_npad >= m).
 *   pg_minkowski_knn       result of pg_f16_knn(pg_minkowski_dense(...)): ranks first..first+k-1 of every Y row's
 *                          (value, column) order over the n X vectors, descending values when similarity != 0;
 *                          first + k <= 64 (more ranks: pg_minkowski_knn_round); missing ranks idx -1, weight 0.
 *                          idx_out int32 [m*k], w_out fp16 [m*k]
 *   pg_minkowski_eps_slots the epsilon test of pg_f16_eps_* (eps_f16 rounded as there) in ONE distance sweep:
 *                          counts[r] = exact number of matches of row r, its first `cap` matching columns
 *                          (ascending) and fp16 values in slot_idx / slot_w [r*cap ...]  (int32 / fp16 [m*cap])
 *   pg_minkowski_eps_compact  after pg_exclusive_scan(counts) -> indptr: rows with counts <= cap copied from their
 *                          slot into indices / weights at indptr[r]; rows beyond cap are left alone
 *   pg_minkowski_eps_fill_rows  the sweep again for the n_list rows of row_list (int64, e.g. the rows with
 *                          counts > cap from pg_compact_flags), every match written at indptr[row] in ascending
 *                          column order.  Together: the CSR of pg_f16_eps_count/_fill, with one host sync (nnz)
 */
int pg_minkowski_knn(const void *x_packed, int64_t n, int64_t x_npad, const void *y_packed, int64_t m, int64_t y_npad,
                     int d, int similarity, int k, int first, int32_t *idx_out, void *w_out_f16, void *stream);
/*
 * pg_minkowski_knn_round — pg_minkowski_knn beyond 63 neighbours: one more fused sweep per round writes the next k
 * (1..64) ranks of every Y row, the pairs strictly after the row's floor in (value, column) order.  Round 1 is
 * pg_minkowski_knn with first = 1, k = 63.  Floors, exhausted rows (-1) and the output stride ldo exactly as in
 * pg_f16_knn_round: the floor is the previous round's last fp16 weight and index, read with row stride floor_ld.
 */
int pg_minkowski_knn_round(const void *x_packed, int64_t n, int64_t x_npad, const void *y_packed, int64_t m,
                           int64_t y_npad, int d, int similarity, int k, const int32_t *floor_idx,
                           const void *floor_w_f16, int64_t floor_ld, int32_t *idx_out, void *w_out_f16, int64_t ldo,
                           void *stream);
int pg_minkowski_eps_slots(const void *x_packed, int64_t n, int64_t x_npad, const void *y_packed, int64_t m,
                           int64_t y_npad, int d, int similarity, int cmp, float eps_f16, int cap, int32_t *slot_idx,
                           void *slot_w_f16, uint32_t *counts, void *stream);
int pg_minkowski_eps_compact(int64_t m, int cap, const int32_t *slot_idx, const void *slot_w_f16, const uint32_t *counts,
                             const int64_t *indptr, int32_t *indices, void *weights_f16, void *stream);
int pg_minkowski_eps_fill_rows(const void *x_packed, int64_t n, int64_t x_npad, const void *y_packed, int64_t m,
                               int64_t y_npad, int d, int similarity, int cmp, float eps_f16, const int64_t *row_list,
                               int64_t n_list, const int64_t *indptr, int32_t *indices, void *weights_f16, void *stream);

/*
 * Cosine graphs of fp16 embeddings on the matrix cores: `build_graph(representation="Embedded",
 * distance=cosine)`.  The reference exports `cosine` without implementing it; the arithmetic is this library's
 * contract (prograph_amd/csrc/pg_cos.hip).  Operands are pg_pack_f16 buffers (x_npad a multiple
 * of 256, y_npad >= m) plus their pg_cosine_prep norms; p, nx and ny are fp32 sums of exact fp16 products from
 * one v_mfma_f32_32x32x16_f16 tile routine in a fixed K order, and
 *   d = 1 if nx == 0 or ny == 0;  else 0 if p == nx == ny bitwise;  else clamp(1 - (p*ry)*rx, 0, 2)  (fp32 steps),
 *   similarity != 0: s = 1/(1+d);  r = 1/sqrt(n), correctly rounded.
 *   pg_cosine_prep         norms / rnorms fp32 [npad] = n and 1/sqrt(n) of every vector of a packed buffer (n = 0
 *                          past the end); flags uint32[1] set to 1 when one of the first n vectors holds an inf or
 *                          nan (the caller must not use the distances then)
 *   pg_cosine_dense        out[m*ldo + n] = fp32 distance (similarity != 0: 1/(1+d)) of Y[m] and X[n]
 *   pg_cosine_knn          ranks first..first+k-1 of every Y row's (value, column) order over the n X vectors of
 *                          that block, descending values when similarity != 0, ties by ascending column;
 *                          first + k <= 64 (more ranks: pg_cosine_knn_round); missing ranks idx -1, weight 0.
 *                          idx_out int32 [m*k], w_out fp32 [m*k]
 *   pg_cosine_eps_slots    comp(d, eps) & (d > 0)  [similarities: comp(eps, s) & (s < 1)], eps an fp32 value, in
 *                          ONE sweep: counts[r] = exact number of matches of row r, its first `cap` matching columns
 *                          (ascending) and values in slot_idx / slot_w [r*cap ...]  (int32 / fp32 [m*cap])
 *   pg_cosine_eps_compact  after pg_exclusive_scan(counts) -> indptr: rows with counts <= cap copied from their slot
 *                          into indices / weights at indptr[r]; rows beyond cap are left alone
 *   pg_cosine_eps_fill_rows  the sweep again for the n_list rows of row_list (int64, e.g. the rows with counts > cap
 *                          from pg_compact_flags), every match written at indptr[row] in ascending column order.
 *                          Together: the CSR of thresholding pg_cosine_dense, with one host sync (nnz)
 * The dense and the fused kernels share the tile routine and the epilogue: their results are equal bit for bit.
 */
int pg_cosine_prep(const void *packed, int64_t n, int64_t npad, int d, float *norms, float *rnorms, uint32_t *flags,
                   void *stream);
int pg_cosine_dense(const void *x_packed, const float *x_norms, const float *x_rnorms, int64_t n, int64_t x_npad,
                    const void *y_packed, const float *y_norms, const float *y_rnorms, int64_t m, int64_t y_npad, int d,
                    int similarity, float *out, int64_t ldo, void *stream);
int pg_cosine_knn(const void *x_packed, const float *x_norms, const float *x_rnorms, int64_t n, int64_t x_npad,
                  const void *y_packed, const float *y_norms, const float *y_rnorms, int64_t m, int64_t y_npad, int d,
                  int similarity, int k, int first, int32_t *idx_out, float *w_out, void *stream);
/*
 * pg_cosine_knn_round — pg_cosine_knn beyond 63 neighbours, as pg_minkowski_knn_round: one more fused sweep per
 * round writes the next k (1..64) ranks of every Y row after its floor.  The floor is the previous round's last
 * fp32 weight and index (floor_w / floor_idx, row stride floor_ld): fp32 values pass through unchanged, so the
 * weight gives the key back exactly.  Exhausted rows (floor index -1) and the output stride ldo as in
 * pg_f16_knn_round.
 */
int pg_cosine_knn_round(const void *x_packed, const float *x_norms, const float *x_rnorms, int64_t n, int64_t x_npad,
                        const void *y_packed, const float *y_norms, const float *y_rnorms, int64_t m, int64_t y_npad, int d,
                        int similarity, int k, const int32_t *floor_idx, const float *floor_w, int64_t floor_ld,
                        int32_t *idx_out, float *w_out, int64_t ldo, void *stream);
int pg_cosine_eps_slots(const void *x_packed, const float *x_norms, const float *x_rnorms, int64_t n, int64_t x_npad,
                        const void *y_packed, const float *y_norms, const float *y_rnorms, int64_t m, int64_t y_npad, int d,
                        int similarity, int cmp, float eps, int cap, int32_t *slot_idx, float *slot_w, uint32_t *counts,
                        void *stream);
int pg_cosine_eps_compact(int64_t m, int cap, const int32_t *slot_idx, const float *slot_w, const uint32_t *counts,
                          const int64_t *indptr, int32_t *indices, float *weights, void *stream);
int pg_cosine_eps_fill_rows(const void *x_packed, const float *x_norms, const float *x_rnorms, int64_t n, int64_t x_npad,
                            const void *y_packed, const float *y_norms, const float *y_rnorms, int64_t m, int64_t y_npad,
                            int d, int similarity, int cmp, float eps, const int64_t *row_list, int64_t n_list,
                            const int64_t *indptr, int32_t *indices, float *weights, void *stream);

/*
 * Euclidean graphs of fp16 embeddings on the matrix cores: `build_graph(representation="Embedded",
 * distance=euclidean)` (prograph_amd/csrc/pg_cos.hip).  The same kernels as the cosine entries with
 * another epilogue on the same three fp32 sums p, nx, ny:
 *   d = 0 if p == nx == ny bitwise (identical vectors, two zero vectors);
 *       else sqrt(max((nx + ny) - (p + p), 0)), every step rounded to fp32, the root correctly rounded;
 *   similarity != 0: s = 1/(1+d).  A zero vector is an ordinary point: d(0, y) = sqrt(ny).
 * Stated tolerance against the exact d^2 of the fp16 values:  |d^2 - exact| <= B(D)(nx + ny) + 2^-22 exact,
 * B(D) = 2 D 2^-24 + 2^-21: the form cancels, so a non-identical pair closer than that may come out as 0.
 * Each entry has the argument list, the checks and the output of its pg_cosine_* twin; the operands are pg_pack_f16
 * buffers with their pg_cosine_prep norms (the rnorms arrays must be given and are not read; the caller checks the
 * non-finite flag).  There is no pg_euclidean_eps_compact: pg_cosine_eps_compact moves slots whatever metric filled
 * them, so the Euclidean CSR is pg_euclidean_eps_slots, pg_exclusive_scan, pg_cosine_eps_compact and
 * pg_euclidean_eps_fill_rows.
 */
int pg_euclidean_dense(const void *x_packed, const float *x_norms, const float *x_rnorms, int64_t n, int64_t x_npad,
                       const void *y_packed, const float *y_norms, const float *y_rnorms, int64_t m, int64_t y_npad, int d,
                       int similarity, float *out, int64_t ldo, void *stream);
int pg_euclidean_knn(const void *x_packed, const float *x_norms, const float *x_rnorms, int64_t n, int64_t x_npad,
                     const void *y_packed, const float *y_norms, const float *y_rnorms, int64_t m, int64_t y_npad, int d,
                     int similarity, int k, int first, int32_t *idx_out, float *w_out, void *stream);
int pg_euclidean_knn_round(const void *x_packed, const float *x_norms, const float *x_rnorms, int64_t n, int64_t x_npad,
                           const void *y_packed, const float *y_norms, const float *y_rnorms, int64_t m, int64_t y_npad,
                           int d, int similarity, int k, const int32_t *floor_idx, const float *floor_w, int64_t floor_ld,
                           int32_t *idx_out, float *w_out, int64_t ldo, void *stream);
int pg_euclidean_eps_slots(const void *x_packed, const float *x_norms, const float *x_rnorms, int64_t n, int64_t x_npad,
                           const void *y_packed, const float *y_norms, const float *y_rnorms, int64_t m, int64_t y_npad,
                           int d, int similarity, int cmp, float eps, int cap, int32_t *slot_idx, float *slot_w,
                           uint32_t *counts, void *stream);
int pg_euclidean_eps_fill_rows(const void *x_packed, const float *x_norms, const float *x_rnorms, int64_t n, int64_t x_npad,
                               const void *y_packed, const float *y_norms, const float *y_rnorms, int64_t m, int64_t y_npad,
                               int d, int similarity, int cmp, float eps, const int64_t *row_list, int64_t n_list,
                               const int64_t *indptr, int32_t *indices, float *weights, void *stream);

/*
 * Multi-GPU: the path's ONE collective (e).  The N^2 pair space shards row-block
 * wise, one process per GPU; every rank needs the whole token matrix, so the ranks all-gather their
 * row shards once (RCCL over xGMI: 64 MB at N = 1M, L = 64) and never talk again.  The reference has
 * no counterpart (single hard-coded cuda:0, prograph/prograph.py:726).
 *   pg_comm_unique_id   rank 0 creates the 128-byte id (ncclGetUniqueId); the host carries it to the
 *                       other ranks by its own means (MPI, a file, torch.distributed's store, ...)
 *   pg_comm_init        every rank, on its GPU (the current HIP device): ncclCommInitRank
 *   pg_allgather_tokens shard (rows_per_rank, l) uint8, contiguous, the same rows_per_rank on every
 *                       rank (pad the last block with zero rows); full (nranks*rows_per_rank, l);
 *                       enqueued on `stream`, no host synchronisation
 * RCCL is resolved at run time (the copy the host process already loaded, else the ROCm installation's):
 * a host without librccl.so still loads this library and gets PG_E_COMM from these calls only.
 *   pg_comm_available   1 when this process can bind RCCL (a local check, no communication): hosts let every rank
 *                       agree on it BEFORE anybody enters the collective pg_comm_init
 */
#define PG_COMM_ID_BYTES 128
int pg_comm_available(void);
int pg_comm_unique_id(void *id128);
int pg_comm_init(void **comm, int nranks, int rank, const void *id128);
int pg_comm_destroy(void *comm);
int pg_allgather_tokens(void *comm, const void *shard, int64_t rows_per_rank, int l, void *full, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PROGRAPH_HIP_H */
