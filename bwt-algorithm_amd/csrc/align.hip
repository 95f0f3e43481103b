// align.hip -- base-level alignment of chains on the device: a banded
// edit-distance DP with traceback per inter-anchor gap, stitched into one CIGAR
// per chain (contract: include/bwtmi.h, bwtmi_index_align_chains).
//
// The host validates the chains and turns them into one descriptor per member:
// member t of a chain (not its first) owns the gap in front of it and the block
// of '=' that it is, so gap and block are indexed by member, never searched for.
// A gap's class is decided there, by its sides alone:
//   none     m = n = 0: nothing between the blocks
//   trivial  m = 0, n = 0 or m = n = 1: no DP, k_align_trace writes the one
//            operation (the 1 x 1 case from one byte compare)
//   small    both sides <= 16: k_align_small, one lane per gap, the row and the
//            text bytes in registers
//   wave     the rest: k_align_wave, one workgroup of one wave per gap
// The work per gap spans four orders of magnitude (1 x 1 next to thousands by
// hundreds), hence the classes.
//   k_align_small   the contract's recurrence, cell by cell, indexed by (i, j)
//   k_align_wave    row by row over the band's columns c = j - i - lo; a lane owns
//                   the columns c, c + 64, ...  The diagonal and the vertical
//                   candidate, t[c] = min(prev[c] + neq, prev[c + 1] + 1), need no
//                   neighbour of the new row; the horizontal one is then D[c] = c +
//                   prefixmin(t[c'] - c'), one wave prefix-min per 64 columns and a
//                   carry between chunks.  Two rows, in LDS up to 1023 columns,
//                   else in global scratch
//   directions      one byte per cell, written by the forward pass with the
//                   contract's preference: 0 diagonal '=', 1 diagonal 'X', 2
//                   left, 3 up.  Row 0 and column 0 are not stored: the
//                   traceback knows them
//   k_align_trace   one lane per gap walks from (m, n), at most m + n dependent
//                   byte loads, and writes run-length operations backwards from
//                   the end of the gap's region (m + n operations at most)
//   k_align_stitch  one lane per chain: blocks and gaps in order, adjacent equal
//                   operations merged.  Run twice: it counts (and sums nm, n_eq,
//                   cols), exclusive_scan<uint32_t> gives the CIGAR offsets, it
//                   writes
// Every loop bound of k_align_wave (m, the band, the chunk range of a row) comes
// from the gap's descriptor at a wave-uniform address: no lane leaves a loop on a
// cross-lane value (Guard).  The other kernels have no cross-lane
// operation at all.
//
// bwtmi_index_align_extend adds, per chain, a head and a tail: a scored banded DP
// with X-drop from each outer anchor towards the read's end.
//   k_extend_score  one wave per extension, score only: the best cell and the
//                   rows computed; the X-drop exit is on a scalar
//   host            reads the best cells: the cap on the whole call's cells, the
//                   spans, and each extension's offsets into the directions (one
//                   byte per cell of the rows up to the best cell's) and the
//                   operations
//   k_extend_dirs   the same rows again, up to the best cell's, directions stored
//   k_extend_trace  one lane per extension, from the best cell to (0, 0)
//   k_align_stitch  takes the head's and the tail's operations as two more runs
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "device.h"

namespace bwtmi {

namespace {

constexpr int kAlignSmall = 16;            // the largest side of a one-lane gap
constexpr int kAlignLdsRow = 1024;         // ints per LDS row: bands of up to 1023 columns (and the sentinel)
constexpr int32_t kAlignInf = 1 << 29;     // no cell: above every distance (<= 131,070), and 2 * kAlignInf fits
constexpr int32_t kAlignMaxSide = 65535;
constexpr int kGapNone = 0, kGapTrivial = 1, kGapSmall = 2, kGapWave = 3;

struct AlignGap {
    int64_t qa;         // a[i] is the query blob's byte qa + i, or on strand 1 the complement of byte qa - i
    int64_t rb;         // b[j] = T[rb + j]
    int64_t dir;        // its first direction byte: small (m + 1)(n + 1) bytes by (i, j), wave (m + 1) Wb by (i, c)
    int64_t row;        // wave, more than 1023 columns: its two rows of Wb + 1 ints in the row scratch; else -1
    uint32_t ops_end;   // the end of its region of operations (they are written backwards)
    int32_t m, n;
    int32_t flags;      // bit 0: strand 1; bits 1..2: the class
};
static_assert(sizeof(AlignGap) == 48, "AlignGap layout");

__device__ __forceinline__ uint8_t align_comp(uint8_t c) {
    return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
}
__device__ __forceinline__ uint8_t align_a(const uint8_t *__restrict__ qs, const AlignGap &g, int32_t i) {
    return (g.flags & 1) ? align_comp(qs[g.qa - i]) : qs[g.qa + i];
}

// One lane per gap of at most 16 x 16.  row[j] holds D[i][j] (kAlignInf outside
// the band or past n); the j loop is unrolled, so row and the text bytes stay in
// registers.  The i loop's bound differs by lane; nothing crosses lanes.
__global__ __launch_bounds__(64) void k_align_small(const AlignGap *__restrict__ gaps,
                                                    const uint32_t *__restrict__ list, int64_t nlist,
                                                    const uint8_t *__restrict__ qs,
                                                    const uint8_t *__restrict__ text, int32_t W,
                                                    uint8_t *__restrict__ dir) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nlist) return;
    const AlignGap g = gaps[list[t]];
    const int32_t m = g.m, n = g.n, delta = n - m;
    const int32_t lo = min(0, delta) - W, hi = max(0, delta) + W;
    int32_t row[kAlignSmall + 1];
    uint8_t bq[kAlignSmall];
#pragma unroll
    for (int j = 0; j <= kAlignSmall; ++j) row[j] = (j <= n && j <= hi) ? j : kAlignInf;
#pragma unroll
    for (int j = 0; j < kAlignSmall; ++j) bq[j] = j < n ? text[g.rb + j] : (uint8_t)0;
    uint8_t *d = dir + g.dir;
    const int32_t w = n + 1;
    for (int32_t i = 1; i <= m; ++i) {
        const uint8_t ai = align_a(qs, g, i - 1);
        int32_t diag = row[0];
        row[0] = -i >= lo ? i : kAlignInf;
#pragma unroll
        for (int j = 1; j <= kAlignSmall; ++j) {
            const int32_t up = row[j];
            const int32_t neq = ai != bq[j - 1];
            const int32_t td = diag + neq, tl = row[j - 1] + 1, tu = up + 1;
            const int32_t D = min(td, min(tl, tu));
            const bool inb = j <= n && j - i >= lo && j - i <= hi;
            if (inb) d[i * w + j] = (uint8_t)(td == D ? neq : tl == D ? 2 : 3);
            row[j] = inb ? D : kAlignInf;
            diag = up;
        }
    }
}

// The rows of one wave gap.  rows: two rows, `stride` ints apart, of Wb + 1 ints
// each (entry Wb is a sentinel that stays kAlignInf); row i lives in rows[(i & 1)
// * stride ...].  A cell outside the matrix holds kAlignInf, so a candidate whose
// source does not exist never reproduces a distance.  Row i's cells in the
// matrix are the columns c_lo(i) .. c_hi(i); both bounds fall by at most one per
// row, so the row written two rows ago is stale up to c_hi(i) + 2 at most, and
// the chunks from c_lo(i) to c_hi(i) + 2 rewrite all of it.
__device__ __forceinline__ void align_rows(int32_t *rows, int32_t stride, const AlignGap &g,
                                           const uint8_t *__restrict__ qs, const uint8_t *__restrict__ text,
                                           int32_t W, uint8_t *__restrict__ dir, int lane) {
    const int32_t m = g.m, n = g.n, delta = n - m;
    const int32_t lo = min(0, delta) - W, Wb = max(0, delta) + W - lo + 1;
    for (int32_t c = lane; c <= Wb; c += 64) {
        const int32_t j = lo + c;
        rows[c] = (c < Wb && j >= 0 && j <= n) ? j : kAlignInf;   // row 0: D[0][j] = j
        rows[stride + c] = kAlignInf;
    }
    __syncthreads();
    uint8_t *d = dir + g.dir;
    const uint8_t *b = text + g.rb;
    for (int32_t i = 1; i <= m; ++i) {
        const int32_t *prev = rows + ((i - 1) & 1) * stride;
        int32_t *cur = rows + (i & 1) * stride;
        const uint8_t ai = align_a(qs, g, i - 1);
        const int32_t c_lo = max(0, -i - lo), c_hi = min(Wb - 1, n - i - lo);
        const int32_t c_end = min(Wb - 1, c_hi + 2);
        int32_t carry = kAlignInf;
        for (int32_t k = c_lo >> 6; k <= c_end >> 6; ++k) {
            const int32_t c = (k << 6) + lane;
            const int32_t j = i + lo + c;
            const bool valid = c >= c_lo && c <= c_hi;
            const int32_t p0 = prev[min(c, Wb)], p1 = prev[min(c + 1, Wb)];
            const uint8_t bj = valid && j >= 1 ? b[j - 1] : (uint8_t)0;
            const int32_t neq = ai != bj;
            const int32_t td = j >= 1 ? p0 + neq : kAlignInf;
            int32_t v = (valid ? min(td, p1 + 1) : kAlignInf) - c;
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {   // inclusive prefix-min over the wave
                const int32_t o = __shfl_up(v, s, 64);
                if (lane >= s) v = min(v, o);
            }
            int32_t ex = __shfl_up(v, 1, 64);
            if (lane == 0) ex = kAlignInf;
            ex = min(ex, carry);
            v = min(v, carry);
            carry = __shfl(v, 63, 64);
            const int32_t D = c + v;   // ex + c = D[i][j - 1] + 1
            if (valid) {
                cur[c] = D;
                d[(int64_t)i * Wb + c] = (uint8_t)(td == D ? neq : ex + c == D ? 2 : 3);
            } else if (c < Wb) {
                cur[c] = kAlignInf;
            }
        }
        __syncthreads();   // one wave: the row's stores before the next row's loads
    }
}

// One workgroup of one wave per gap.
__global__ __launch_bounds__(64) void k_align_wave(const AlignGap *__restrict__ gaps,
                                                   const uint32_t *__restrict__ list,
                                                   const uint8_t *__restrict__ qs,
                                                   const uint8_t *__restrict__ text, int32_t W,
                                                   uint8_t *__restrict__ dir, int32_t *__restrict__ rowbuf) {
    __shared__ int32_t lds[2 * kAlignLdsRow];
    const AlignGap g = gaps[list[blockIdx.x]];
    const int lane = (int)threadIdx.x;
    if (g.row < 0) {
        align_rows(lds, kAlignLdsRow, g, qs, text, W, dir, lane);
    } else {
        const int32_t delta = g.n - g.m;
        const int32_t Wb = (delta < 0 ? -delta : delta) + 2 * W + 1;
        align_rows(rowbuf + g.row, Wb + 1, g, qs, text, W, dir, lane);
    }
}

// One lane per member: its gap's operations, run-length, written backwards from
// ops_end; opcnt = how many.
__global__ __launch_bounds__(256) void k_align_trace(const AlignGap *__restrict__ gaps, int64_t ngap,
                                                     const uint8_t *__restrict__ qs,
                                                     const uint8_t *__restrict__ text, int32_t W,
                                                     const uint8_t *__restrict__ dir, uint32_t *__restrict__ ops,
                                                     uint32_t *__restrict__ opcnt) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ngap) return;
    const AlignGap g = gaps[t];
    const int cls = g.flags >> 1;
    if (cls == kGapNone) {
        opcnt[t] = 0;
        return;
    }
    uint32_t *o = ops + g.ops_end;
    const int32_t m = g.m, n = g.n;
    if (cls == kGapTrivial) {
        uint32_t op;
        if (m == 0) op = (uint32_t)n << 4 | 2u;
        else if (n == 0) op = (uint32_t)m << 4 | 1u;
        else op = 1u << 4 | (align_a(qs, g, 0) == text[g.rb] ? 7u : 8u);
        o[-1] = op;
        opcnt[t] = 1;
        return;
    }
    const bool small = cls == kGapSmall;
    const int32_t delta = n - m, lo = min(0, delta) - W, Wb = max(0, delta) + W - lo + 1;
    const uint8_t *d = dir + g.dir;
    int32_t i = m, j = n;
    uint32_t cur = 0, len = 0, cnt = 0;
    while (i > 0 || j > 0) {   // every step lowers i or j: at most m + n steps
        const int64_t at = small ? (int64_t)(i * (n + 1) + j) : (int64_t)i * Wb + (j - i - lo);
        const uint32_t code = i == 0 ? 2u : j == 0 ? 3u : d[at];
        const uint32_t op = code == 0 ? 7u : code == 1 ? 8u : code == 2 ? 2u : 1u;
        if (code != 2) --i;
        if (code != 3) --j;
        if (op == cur) {
            ++len;
        } else {
            if (len) *--o = len << 4 | cur, ++cnt;
            cur = op;
            len = 1;
        }
    }
    if (len) *--o = len << 4 | cur, ++cnt;
    opcnt[t] = cnt;
}

// ---- extension past the outer anchors (contract: include/bwtmi.h, bwtmi_index_align_extend)
// Extension 2k is chain k's head, 2k + 1 its tail.  A head is the tail rule on
// the reversed strings, so a descriptor says which way its bytes run.
struct AlignExt {
    int64_t qa;      // a[i] is the query blob's byte qa + i (flags bit 1: qa - i), complemented on flags bit 0
    int64_t rb;      // b[j] = T[rb + j] (flags bit 2: T[rb - j])
    int32_t m, n;    // m = 0 or n = 0: no extension
    int32_t flags;   // bit 0 complement, bit 1 the query bytes descend, bit 2 the text bytes descend (a head)
    int32_t pad;
};
static_assert(sizeof(AlignExt) == 32, "AlignExt layout");
struct ExtBest {     // k_extend_score's answer
    int32_t bi, bj, score, rows;
};
struct ExtPlan {     // the host's, from the best cells
    int64_t dir;     // its first direction byte: (bi + 1) (2 We + 1) bytes by (i, c); row 0 is not stored
    int64_t ops;     // its region of bi + bj operations
};
struct ExtScore {
    int32_t A, B, G, X, We;
};
constexpr int32_t kExtNeg = -(1 << 29);      // no cell: below every score (>= -2^20 - 4 * 64 * 1024), and 2 * kExtNeg fits

__device__ __forceinline__ uint8_t ext_a(const uint8_t *__restrict__ qs, const AlignExt &e, int32_t i) {
    const uint8_t ch = qs[(e.flags & 2) ? e.qa - i : e.qa + i];
    return (e.flags & 1) ? align_comp(ch) : ch;
}
__device__ __forceinline__ uint8_t ext_b(const uint8_t *__restrict__ text, const AlignExt &e, int32_t j) {
    return text[(e.flags & 4) ? e.rb - j : e.rb + j];
}

// Rows 1 .. R of one extension, on one wave: row i over the band's columns c =
// j - i + We, a lane owns c, c + 64, ...  rows: two rows of 2 We + 2 ints in LDS
// (entry 2 We + 1 is a sentinel that stays kExtNeg); a cell outside the matrix
// holds kExtNeg, so a candidate whose source does not exist never reproduces a
// score.  t[c] = max(prev[c] + s, prev[c + 1] - G) needs no neighbour of the new
// row; the horizontal candidate is then H[c] = -G c + prefixmax(t[c'] + G c'):
// k_align_wave's scan and chunk carry with max for min.  Both bounds of a row
// fall by at most one per row, so (as there) the chunks up to c_hi + 2 rewrite
// all that the row written two rows ago left.
// kStore = false, the score pass: R = every row that has a cell; the row's
//   maximum and its smallest column are one wave reduction of H * 4096 + (4095 -
//   c), taken as scalars (readfirstlane): the best cell, the row count and the
//   X-drop exit are wave-uniform (Guard).  Writes *best.
// kStore = true, the direction pass: R = the best cell's row, no exit; one byte
//   per cell with the gap DP's codes and preference.
template <bool kStore>
__device__ __forceinline__ void extend_rows(int32_t *rows, const AlignExt &e, const uint8_t *__restrict__ qs,
                                            const uint8_t *__restrict__ text, const ExtScore s, int32_t R,
                                            uint8_t *__restrict__ d, ExtBest *__restrict__ out, int lane) {
    const int32_t We = s.We, Wb = 2 * We + 1, stride = Wb + 1, m = e.m, n = e.n;
    for (int32_t c = lane; c <= Wb; c += 64) {
        const int32_t j = c - We;
        rows[c] = (c < Wb && j >= 0 && j <= n) ? -s.G * j : kExtNeg;   // row 0: H[0][j] = -G j
        rows[stride + c] = kExtNeg;
    }
    __syncthreads();
    int32_t best = 0, bi = 0, bj = 0, nrows = 0;
    uint32_t aa = 0;   // a[i - 1 + lane] of the 64 rows from i: one load per 64 rows, one readlane per row
    for (int32_t i = 1; i <= R; ++i) {
        if (((i - 1) & 63) == 0) aa = i - 1 + lane < m ? ext_a(qs, e, i - 1 + lane) : 0u;
        const uint32_t ai = (uint32_t)__builtin_amdgcn_readlane((int)aa, (i - 1) & 63);
        const int32_t *prev = rows + ((i - 1) & 1) * stride;
        int32_t *cur = rows + (i & 1) * stride;
        const int32_t c_lo = max(0, We - i), c_hi = min(Wb - 1, n - i + We);
        const int32_t c_end = min(Wb - 1, c_hi + 2);
        int32_t carry = kExtNeg;
        long long key = INT64_MIN;
        for (int32_t k = c_lo >> 6; k <= c_end >> 6; ++k) {
            const int32_t c = (k << 6) + lane;
            const int32_t j = i + c - We;
            const bool valid = c >= c_lo && c <= c_hi;
            const int32_t p0 = prev[min(c, Wb)], p1 = prev[min(c + 1, Wb)];
            const bool eq = valid && j >= 1 && ai == (uint32_t)ext_b(text, e, j - 1);
            const int32_t td = j >= 1 ? p0 + (eq ? s.A : -s.B) : kExtNeg;
            int32_t v = (valid ? max(td, p1 - s.G) : kExtNeg) + s.G * c;
#pragma unroll
            for (int sh = 1; sh < 64; sh <<= 1) {   // inclusive prefix-max over the wave
                const int32_t o = __shfl_up(v, sh, 64);
                if (lane >= sh) v = max(v, o);
            }
            int32_t ex = __shfl_up(v, 1, 64);
            if (lane == 0) ex = kExtNeg;
            ex = max(ex, carry);
            v = max(v, carry);
            carry = __shfl(v, 63, 64);
            const int32_t H = v - s.G * c;   // ex - G c = H[i][j - 1] - G
            if (valid) {
                cur[c] = H;
                if (kStore) d[(int64_t)i * Wb + c] = (uint8_t)(td == H ? (eq ? 0 : 1) : ex - s.G * c == H ? 2 : 3);
                else key = max(key, (long long)H * 4096 + (4095 - c));
            } else if (c < Wb) {
                cur[c] = kExtNeg;
            }
        }
        if (!kStore) {
#pragma unroll
            for (int sh = 1; sh < 64; sh <<= 1) key = max(key, __shfl_xor(key, sh, 64));
            const long long rk = (long long)__builtin_amdgcn_readfirstlane((int)(key >> 32)) << 32 |
                                 (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)key);
            const int32_t rowmax = (int32_t)(rk >> 12);   // floor: the low 12 bits are 4095 - c >= 0
            nrows = i;
            if (rowmax > best) {   // strictly: ties keep the smaller i, and within the row the key kept the smaller j
                best = rowmax;
                bi = i;
                bj = i + (4095 - (int32_t)(rk & 4095)) - We;
            }
            if (best - rowmax > s.X) break;   // a scalar
        }
        __syncthreads();   // one wave: the row's stores before the next row's loads
    }
    if (!kStore && lane == 0) *out = ExtBest{bi, bj, best, nrows};
}

// One workgroup of one wave per extension: its best cell and its rows.
__global__ __launch_bounds__(64) void k_extend_score(const AlignExt *__restrict__ ext,
                                                     const uint8_t *__restrict__ qs,
                                                     const uint8_t *__restrict__ text, const ExtScore s,
                                                     ExtBest *__restrict__ best) {
    extern __shared__ int32_t lds[];   // the launch's 2 (2 We + 2) ints: 528 bytes at We = 32, 16 KiB at 1024
    const AlignExt e = ext[blockIdx.x];
    const int lane = (int)threadIdx.x;
    if (e.m == 0 || e.n == 0) {
        if (lane == 0) best[blockIdx.x] = ExtBest{0, 0, 0, 0};
        return;
    }
    extend_rows<false>(lds, e, qs, text, s, min(e.m, e.n + s.We), nullptr, best + blockIdx.x, lane);
}

// One workgroup of one wave per extension whose best cell is not (0, 0): the
// directions of the rows up to the best cell's.
__global__ __launch_bounds__(64) void k_extend_dirs(const AlignExt *__restrict__ ext,
                                                    const uint32_t *__restrict__ list,
                                                    const uint8_t *__restrict__ qs,
                                                    const uint8_t *__restrict__ text, const ExtScore s,
                                                    const ExtBest *__restrict__ best,
                                                    const ExtPlan *__restrict__ plan, uint8_t *__restrict__ dir) {
    extern __shared__ int32_t lds[];   // the launch's 2 (2 We + 2) ints: 528 bytes at We = 32, 16 KiB at 1024
    const uint32_t x = list[blockIdx.x];
    extend_rows<true>(lds, ext[x], qs, text, s, best[x].bi, dir + plan[x].dir, nullptr, (int)threadIdx.x);
}

// One lane per listed extension walks from its best cell to (0, 0), at most bi +
// bj dependent byte loads, and writes run-length operations forwards from the
// start of its region: a head's are then in the CIGAR's order (the walk reverses
// the reversed strings' alignment), a tail's in reverse (k_align_stitch reads
// them backwards).  ecnt = how many; an extension not listed keeps its 0.
__global__ __launch_bounds__(256) void k_extend_trace(const uint32_t *__restrict__ list, int64_t nlist, int32_t We,
                                                      const ExtBest *__restrict__ best,
                                                      const ExtPlan *__restrict__ plan,
                                                      const uint8_t *__restrict__ dir, uint32_t *__restrict__ eops,
                                                      uint32_t *__restrict__ ecnt) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nlist) return;
    const uint32_t x = list[t];
    const int32_t Wb = 2 * We + 1;
    const uint8_t *d = dir + plan[x].dir;
    uint32_t *o = eops + plan[x].ops;
    int32_t i = best[x].bi, j = best[x].bj;
    uint32_t cur = 0, len = 0, cnt = 0;
    while (i > 0 || j > 0) {   // every step lowers i or j: at most bi + bj steps
        const uint32_t code = i == 0 ? 2u : d[(int64_t)i * Wb + (j - i + We)];
        const uint32_t op = code == 0 ? 7u : code == 1 ? 8u : code == 2 ? 2u : 1u;
        if (code != 2) --i;
        if (code != 3) --j;
        if (op == cur) {
            ++len;
        } else {
            if (len) o[cnt++] = len << 4 | cur;
            cur = op;
            len = 1;
        }
    }
    if (len) o[cnt++] = len << 4 | cur;
    ecnt[x] = cnt;
}

// One lane per chain.  cigar == nullptr: count the merged operations into nops
// and sum nm, n_eq, cols; else write them at cigar + cig_off[chain].  ecnt !=
// nullptr: the chain's head operations go in front and its tail's behind.
__global__ __launch_bounds__(64) void k_align_stitch(const int64_t *__restrict__ member_off, int64_t nchain,
                                                     const int32_t *__restrict__ blk,
                                                     const AlignGap *__restrict__ gaps,
                                                     const uint32_t *__restrict__ ops,
                                                     const uint32_t *__restrict__ opcnt,
                                                     const ExtPlan *__restrict__ plan,
                                                     const uint32_t *__restrict__ eops,
                                                     const uint32_t *__restrict__ ecnt,
                                                     const uint32_t *__restrict__ cig_off, uint32_t *__restrict__ cigar,
                                                     uint32_t *__restrict__ nops, int32_t *__restrict__ nm,
                                                     int32_t *__restrict__ n_eq, int32_t *__restrict__ cols) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nchain) return;
    const int64_t a = member_off[k], b = member_off[k + 1];
    uint32_t *out = cigar ? cigar + cig_off[k] : nullptr;
    uint32_t cnt = 0, cur = 7u, len = 0, s_eq = 0, s_nm = 0;   // len = 0: nothing to flush yet
    auto flush = [&] {
        if (len == 0) return;
        if (out) out[cnt] = len << 4 | cur;
        ++cnt;
        if (cur == 7u) s_eq += len;
        else s_nm += len;
    };
    auto put = [&](uint32_t op, uint32_t l) {
        if (op == cur) {
            len += l;
        } else {
            flush();
            cur = op;
            len = l;
        }
    };
    if (ecnt) {
        const uint32_t c = ecnt[2 * k];
        const uint32_t *o = eops + plan[2 * k].ops;
        for (uint32_t x = 0; x < c; ++x) put(o[x] & 15u, o[x] >> 4);
    }
    put(7u, (uint32_t)blk[a]);
    for (int64_t t = a + 1; t < b; ++t) {
        const uint32_t c = opcnt[t];
        const uint32_t *o = ops + gaps[t].ops_end - c;
        for (uint32_t x = 0; x < c; ++x) put(o[x] & 15u, o[x] >> 4);
        put(7u, (uint32_t)blk[t]);
    }
    if (ecnt) {
        const uint32_t c = ecnt[2 * k + 1];
        const uint32_t *o = eops + plan[2 * k + 1].ops;
        for (uint32_t x = c; x-- > 0;) put(o[x] & 15u, o[x] >> 4);
    }
    flush();
    if (!out) {
        nops[k] = cnt;
        nm[k] = (int32_t)s_nm;
        n_eq[k] = (int32_t)s_eq;
        cols[k] = (int32_t)(s_nm + s_eq);
    }
}

// carves one slot into arrays (256-byte aligned)
struct AlignArena {
    size_t used = 0;
    uint8_t *base = nullptr;
    size_t take(size_t bytes) {
        const size_t at = used;
        used += (bytes + 255) & ~size_t{255};
        return at;
    }
    template <class T> T *at(size_t off) const { return reinterpret_cast<T *>(base + off); }
};

void align_fail_cells(AlignResult &out, int64_t cells, int64_t max_cells) {
    out.aq_start.clear();
    out.aq_end.clear();
    out.ar_start.clear();
    out.ar_end.clear();
    fail(BWTMI_E_NOMEM, "align: %lld DP cells exceed max_cells %lld", (long long)cells, (long long)max_cells);
}

// Both entries: ep == nullptr is bwtmi_index_align_chains, whose launches and
// arrays the extension leaves as they are.
void align_run(Ctx &c, DeviceIndex *ix, const uint8_t *qs, const int64_t *off, int64_t nq, const int64_t *chain_off,
               const uint8_t *strand, const int64_t *member_off, const int32_t *mq, const int64_t *mr,
               const int32_t *mlen, int64_t nchain, int64_t nmember, const AlignParams &p, const ExtendParams *ep,
               AlignResult &out) {
    out = AlignResult{};
    // ---- validation and the descriptors: nothing reaches the device before the last check
    if (nq < 0 || nchain < 0 || nmember < 0 || !off || !chain_off || !member_off)
        fail(BWTMI_E_ARG, "align: negative count or null offsets");
    if ((nchain > 0 && !strand) || (nmember > 0 && !(mq && mr && mlen))) fail(BWTMI_E_ARG, "align: null chain array");
    if (p.band < 0 || p.band > 1024) fail(BWTMI_E_ARG, "align: band %d outside 0..1024", (int)p.band);
    if (ep) {
        if (ep->ext_band < 0 || ep->ext_band > 1024)
            fail(BWTMI_E_ARG, "align: ext_band %d outside 0..1024", (int)ep->ext_band);
        if (ep->match < 1 || ep->match > 64) fail(BWTMI_E_ARG, "align: match %d outside 1..64", (int)ep->match);
        if (ep->mismatch < 0 || ep->mismatch > 64)
            fail(BWTMI_E_ARG, "align: mismatch %d outside 0..64", (int)ep->mismatch);
        if (ep->gap < 1 || ep->gap > 64) fail(BWTMI_E_ARG, "align: gap %d outside 1..64", (int)ep->gap);
        if (ep->xdrop < 0 || ep->xdrop > (1 << 20)) fail(BWTMI_E_ARG, "align: xdrop %d outside 0..2^20", (int)ep->xdrop);
        if (nchain >= (int64_t{1} << 30))
            fail(BWTMI_E_NOMEM, "align: %lld chains have 2^31 extensions and more", (long long)nchain);
    }
    if (nchain >= (int64_t{1} << 31) || nmember >= (int64_t{1} << 31))
        fail(BWTMI_E_NOMEM, "align: %lld chains of %lld members exceed the 2^31 the aligner indexes", (long long)nchain,
             (long long)nmember);
    for (int64_t i = 0; i < nq; ++i)
        if (off[i + 1] < off[i]) fail(BWTMI_E_ARG, "align: query offsets decrease at query %lld", (long long)i);
    if (chain_off[0] != 0 || chain_off[nq] != nchain)
        fail(BWTMI_E_ARG, "align: chain_off must run from 0 to nchain %lld", (long long)nchain);
    for (int64_t i = 0; i < nq; ++i)
        if (chain_off[i + 1] < chain_off[i]) fail(BWTMI_E_ARG, "align: chain_off decreases at query %lld", (long long)i);
    if (member_off[0] != 0 || member_off[nchain] != nmember)
        fail(BWTMI_E_ARG, "align: member_off must run from 0 to nmember %lld", (long long)nmember);
    const int64_t tn = index_n(ix), q0 = off[0];
    const int32_t W = p.band;
    if (qs == nullptr && off[nq] > q0) fail(BWTMI_E_ARG, "align: null queries");

    const size_t C = (size_t)nchain, M = (size_t)nmember;
    std::vector<AlignGap> gaps(M);
    std::vector<int32_t> blk(M);
    std::vector<uint32_t> small, wave;
    std::vector<AlignExt> ext(ep ? 2 * C : 0);
    const int32_t We = ep ? ep->ext_band : 0;
    out.aq_start.resize(C);
    out.aq_end.resize(C);
    out.ar_start.resize(C);
    out.ar_end.resize(C);
    int64_t cells = 0, dir_bytes = 0, row_ints = 0, ops_total = 0;
    for (int64_t qi = 0; qi < nq; ++qi) {
        const int64_t qlen = off[qi + 1] - off[qi];
        if (chain_off[qi + 1] > chain_off[qi] && qlen >= (int64_t{1} << 28))
            fail(BWTMI_E_ARG, "align: query %lld has %lld bytes, 2^28 and more", (long long)qi, (long long)qlen);
        for (int64_t k = chain_off[qi]; k < chain_off[qi + 1]; ++k) {
            const int64_t a = member_off[k], b = member_off[k + 1];
            if (b <= a || b > nmember)
                fail(BWTMI_E_ARG, "align: chain %lld has no member (or member_off leaves 0 .. nmember)", (long long)k);
            if (strand[k] > 1) fail(BWTMI_E_ARG, "align: chain %lld has strand %d", (long long)k, (int)strand[k]);
            const bool rev = strand[k] != 0;
            int64_t qe_prev = 0, re_prev = 0, sq0 = 0;
            for (int64_t t = a; t < b; ++t) {
                const int64_t len = mlen[t], oq = mq[t], r = mr[t];
                if (len < 1 || oq < 0 || oq + len > qlen || r < 0 || r + len > tn)
                    fail(BWTMI_E_ARG, "align: member %lld (q %lld, r %lld, len %lld) outside len >= 1, its query of %lld "
                         "bytes or the text of %lld", (long long)t, (long long)oq, (long long)r, (long long)len,
                         (long long)qlen, (long long)tn);
                const int64_t sq = rev ? qlen - oq - len : oq, qe = sq + len, re = r + len;
                AlignGap &g = gaps[(size_t)t];
                g = AlignGap{0, 0, 0, -1, 0, 0, 0, (rev ? 1 : 0) | kGapNone << 1};
                if (t == a) {
                    blk[(size_t)t] = (int32_t)len;
                    sq0 = sq;
                    out.ar_start[(size_t)k] = r;
                } else {
                    const int64_t dq = qe - qe_prev, dr = re - re_prev;
                    if (dq <= 0 || dr <= 0)
                        fail(BWTMI_E_ARG, "align: member %lld does not end after its predecessor (dq %lld, dr %lld)",
                             (long long)t, (long long)dq, (long long)dr);
                    const int64_t tt = std::min(len, std::min(dq, dr)), m = dq - tt, n = dr - tt;
                    if (m > kAlignMaxSide || n > kAlignMaxSide)
                        fail(BWTMI_E_ARG, "align: the gap in front of member %lld is %lld x %lld, a side above 65535",
                             (long long)t, (long long)m, (long long)n);
                    blk[(size_t)t] = (int32_t)tt;
                    g.m = (int32_t)m;
                    g.n = (int32_t)n;
                    g.qa = (off[qi] - q0) + (rev ? qlen - 1 - qe_prev : qe_prev);
                    g.rb = re_prev;
                    const int64_t wb = (n > m ? n - m : m - n) + 2 * W + 1;
                    int cls = kGapNone;
                    if (m > 0 && n > 0) {
                        const int64_t cg = (m + 1) * wb;
                        cells = cells > INT64_MAX - cg ? INT64_MAX : cells + cg;
                    }
                    if (m == 0 && n == 0) {
                        cls = kGapNone;
                    } else if (m == 0 || n == 0 || (m == 1 && n == 1)) {
                        cls = kGapTrivial;
                        ++out.gaps[0];
                        ops_total += 1;
                    } else if (m <= kAlignSmall && n <= kAlignSmall) {
                        cls = kGapSmall;
                        ++out.gaps[1];
                        small.push_back((uint32_t)t);
                        g.dir = dir_bytes;
                        dir_bytes += (m + 1) * (n + 1);
                        ops_total += m + n;
                    } else {
                        cls = kGapWave;
                        ++out.gaps[2];
                        wave.push_back((uint32_t)t);
                        g.dir = dir_bytes;
                        dir_bytes += (m + 1) * wb;   // (<= this gap's cells: the cap below bounds the sum)
                        if (wb + 1 > kAlignLdsRow) {
                            g.row = row_ints;
                            row_ints += 2 * (wb + 1);
                        }
                        ops_total += m + n;
                    }
                    g.flags = (rev ? 1 : 0) | cls << 1;
                    if (ops_total >= (int64_t{1} << 32))
                        fail(BWTMI_E_NOMEM, "align: the gaps' sides sum to 2^32 operations and more");
                    g.ops_end = (uint32_t)ops_total;
                }
                qe_prev = qe;
                re_prev = re;
            }
            if (re_prev - out.ar_start[(size_t)k] >= (int64_t{1} << 30))
                fail(BWTMI_E_ARG, "align: chain %lld spans %lld text bytes, 2^30 and more", (long long)k,
                     (long long)(re_prev - out.ar_start[(size_t)k]));
            out.ar_end[(size_t)k] = re_prev;
            out.aq_start[(size_t)k] = (int32_t)(rev ? qlen - qe_prev : sq0);
            out.aq_end[(size_t)k] = (int32_t)(rev ? qlen - sq0 : qe_prev);
            if (ep) {
                if (qlen * ep->match >= (int64_t{1} << 30))
                    fail(BWTMI_E_ARG, "align: query %lld of %lld bytes at match %d: a score of 2^30 and more",
                         (long long)qi, (long long)qlen, (int)ep->match);
                const int64_t base = off[qi] - q0, r0 = out.ar_start[(size_t)k];
                const int64_t hm = sq0, tm = qlen - qe_prev;
                ext[2 * (size_t)k] = AlignExt{base + (rev ? qlen - sq0 : sq0 - 1), r0 - 1, (int32_t)hm,
                                              (int32_t)std::min(r0, hm + We), (rev ? 1 : 2) | 4, 0};
                ext[2 * (size_t)k + 1] = AlignExt{base + (rev ? qlen - 1 - qe_prev : qe_prev), re_prev, (int32_t)tm,
                                                  (int32_t)std::min(tn - re_prev, tm + We), rev ? 3 : 0, 0};
            }
        }
    }
    out.cells_total = cells;
    if (cells > p.max_cells) align_fail_cells(out, cells, p.max_cells);
    out.cigar_off.assign(C + 1, 0);
    if (nchain == 0) return;

    // ---- one slot, carved; the directions, the wide rows and the CIGARs have slots of their own
    const size_t qbytes = (size_t)(off[nq] - q0);
    AlignArena ar;
    const size_t o_qs = ar.take(qbytes + 1), o_gaps = ar.take(M * sizeof(AlignGap)), o_blk = ar.take(M * 4);
    const size_t o_moff = ar.take((C + 1) * 8), o_small = ar.take(small.size() * 4 + 4), o_wave = ar.take(wave.size() * 4 + 4);
    const size_t o_opcnt = ar.take(M * 4), o_ops = ar.take((size_t)ops_total * 4 + 4);
    const size_t o_nops = ar.take((C + 1) * 4), o_coff = ar.take((C + 1) * 4);
    const size_t o_nm = ar.take(C * 4), o_neq = ar.take(C * 4), o_cols = ar.take(C * 4);
    const size_t E = ext.size();   // 2 C, or 0 without extension
    const size_t o_ext = ar.take(E * sizeof(AlignExt)), o_best = ar.take(E * sizeof(ExtBest));
    const size_t o_plan = ar.take(E * sizeof(ExtPlan)), o_elist = ar.take(E * 4 + 4), o_ecnt = ar.take(E * 4);
    c.slot[S_IDX0].ensure(ar.used);
    c.slot[S_IDX2].ensure((size_t)dir_bytes + 1);
    c.slot[S_IDX3].ensure((size_t)row_ints * 4 + 4);
    ar.base = c.slot[S_IDX0].as<uint8_t>();
    uint8_t *d_qs = ar.at<uint8_t>(o_qs), *d_dir = c.slot[S_IDX2].as<uint8_t>();
    AlignGap *d_gaps = ar.at<AlignGap>(o_gaps);
    int32_t *d_blk = ar.at<int32_t>(o_blk), *d_rows = c.slot[S_IDX3].as<int32_t>();
    int64_t *d_moff = ar.at<int64_t>(o_moff);
    uint32_t *d_small = ar.at<uint32_t>(o_small), *d_wave = ar.at<uint32_t>(o_wave), *d_opcnt = ar.at<uint32_t>(o_opcnt);
    uint32_t *d_ops = ar.at<uint32_t>(o_ops), *d_nops = ar.at<uint32_t>(o_nops), *d_coff = ar.at<uint32_t>(o_coff);
    int32_t *d_nm = ar.at<int32_t>(o_nm), *d_neq = ar.at<int32_t>(o_neq), *d_cols = ar.at<int32_t>(o_cols);
    const uint8_t *d_text = index_text_device(ix);
    AlignExt *d_ext = ar.at<AlignExt>(o_ext);
    ExtBest *d_best = ar.at<ExtBest>(o_best);
    ExtPlan *d_plan = ar.at<ExtPlan>(o_plan);
    uint32_t *d_elist = ar.at<uint32_t>(o_elist), *d_ecnt = ar.at<uint32_t>(o_ecnt);

    hipStream_t st = c.stream;
    // timed like a kernel (statistics name align_upload): what the chains' way back up costs
    c.kbegin("align_upload", (double)qbytes + (double)M * (sizeof(AlignGap) + 4) + (double)(C + 1) * 8);
    if (qbytes) HIPCHECK(hipMemcpyAsync(d_qs, qs + q0, qbytes, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_gaps, gaps.data(), M * sizeof(AlignGap), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_blk, blk.data(), M * 4, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_moff, member_off, (C + 1) * 8, hipMemcpyHostToDevice, st));
    if (!small.empty()) HIPCHECK(hipMemcpyAsync(d_small, small.data(), small.size() * 4, hipMemcpyHostToDevice, st));
    if (!wave.empty()) HIPCHECK(hipMemcpyAsync(d_wave, wave.data(), wave.size() * 4, hipMemcpyHostToDevice, st));
    if (E) HIPCHECK(hipMemcpyAsync(d_ext, ext.data(), E * sizeof(AlignExt), hipMemcpyHostToDevice, st));
    c.kend();
    HIPCHECK(hipMemsetAsync(d_nops + C, 0, 4, st));

    // ---- the extensions' score pass goes first: the host plans the second pass behind the gaps' kernels
    const size_t ext_lds = 2 * (2 * (size_t)We + 2) * sizeof(int32_t);
    const ExtScore es{ep ? ep->match : 0, ep ? ep->mismatch : 0, ep ? ep->gap : 0, ep ? ep->xdrop : 0, We};
    if (ep) {
        KLAUNCH("k_extend_score", (double)E * (sizeof(AlignExt) + sizeof(ExtBest)), k_extend_score, dim3((unsigned)E),
                dim3(64), ext_lds, st, d_ext, d_qs, d_text, es, d_best);
        HIPCHECK(hipGetLastError());
    }

    // ---- the gaps: forward passes by class, then every member's traceback
    if (!small.empty()) {
        const int64_t ns = (int64_t)small.size();
        KLAUNCH("k_align_small", (double)ns * 64.0, k_align_small, dim3(blocks(ns, 64)), dim3(64), 0, st, d_gaps, d_small,
                ns, d_qs, d_text, W, d_dir);
        HIPCHECK(hipGetLastError());
    }
    if (!wave.empty()) {
        KLAUNCH("k_align_wave", (double)dir_bytes, k_align_wave, dim3((unsigned)wave.size()), dim3(64), 0, st, d_gaps,
                d_wave, d_qs, d_text, W, d_dir, d_rows);
        HIPCHECK(hipGetLastError());
    }
    KLAUNCH("k_align_trace", (double)nmember * 52.0 + (double)ops_total * 4.0, k_align_trace, dim3(blocks(nmember)),
            dim3(256), 0, st, d_gaps, nmember, d_qs, d_text, W, d_dir, d_ops, d_opcnt);
    HIPCHECK(hipGetLastError());

    // ---- the extensions: best cells down, the cap, the plan up, directions, traceback
    const ExtPlan *s_plan = nullptr;     // what k_align_stitch gets: nothing without extension
    const uint32_t *s_eops = nullptr, *s_ecnt = nullptr;
    int64_t eops_total = 0;
    std::vector<ExtPlan> plan(E);
    std::vector<uint32_t> elist;
    if (ep) {
        ExtBest *hb = c.mailbox<ExtBest>(E);
        HIPCHECK(hipMemcpyAsync(hb, d_best, E * sizeof(ExtBest), hipMemcpyDeviceToHost, st));
        scan_wait(st);   // (the gaps' kernels are done too: their directions' slot is free)
        const int64_t Wb = 2 * (int64_t)We + 1;
        int64_t edir = 0, ecells = 0;
        out.head_score.resize(C);
        out.tail_score.resize(C);
        for (size_t x = 0; x < E; ++x) {
            const ExtBest b = hb[x];
            const AlignExt &e = ext[x];
            if (b.bi < 0 || b.bi > e.m || b.bj < 0 || b.bj > e.n || b.rows < b.bi || (b.bi == 0 && b.bj != 0))
                fail(BWTMI_E_STATE, "align: extension %lld ends at (%d, %d) of %d x %d", (long long)x, (int)b.bi,
                     (int)b.bj, (int)e.m, (int)e.n);
            plan[x] = ExtPlan{edir, eops_total};
            out.ext_rows += b.rows;
            if (e.m > 0 && e.n > 0) {
                const int64_t ce = ((int64_t)b.bi + 1) * Wb;
                ecells = ecells > INT64_MAX - ce ? INT64_MAX : ecells + ce;
            }
            if (b.bi > 0) {
                elist.push_back((uint32_t)x);
                edir += ((int64_t)b.bi + 1) * Wb;
                eops_total += (int64_t)b.bi + b.bj;
            }
            const size_t k = x >> 1;
            const bool rev = strand[k] != 0;
            if (x & 1) {   // a tail lengthens the searched string's end, a head its start
                out.tail_score[k] = b.score;
                (rev ? out.aq_start[k] : out.aq_end[k]) += rev ? -b.bi : b.bi;
                out.ar_end[k] += b.bj;
            } else {
                out.head_score[k] = b.score;
                (rev ? out.aq_end[k] : out.aq_start[k]) += rev ? b.bi : -b.bi;
                out.ar_start[k] -= b.bj;
            }
        }
        cells = cells > INT64_MAX - ecells ? INT64_MAX : cells + ecells;
        out.cells_total = cells;
        if (cells > p.max_cells) {
            out.head_score.clear();
            out.tail_score.clear();
            out.cigar_off.clear();
            align_fail_cells(out, cells, p.max_cells);
        }
        c.slot[S_IDX2].ensure((size_t)edir + 1);   // (<= the extensions' cells)
        c.slot[S_IDX4].ensure((size_t)eops_total * 4 + 4);
        uint8_t *d_edir = c.slot[S_IDX2].as<uint8_t>();
        uint32_t *d_eops = c.slot[S_IDX4].as<uint32_t>();
        HIPCHECK(hipMemcpyAsync(d_plan, plan.data(), E * sizeof(ExtPlan), hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemsetAsync(d_ecnt, 0, E * 4, st));
        if (!elist.empty()) {
            const int64_t nl = (int64_t)elist.size();
            HIPCHECK(hipMemcpyAsync(d_elist, elist.data(), elist.size() * 4, hipMemcpyHostToDevice, st));
            KLAUNCH("k_extend_dirs", (double)edir, k_extend_dirs, dim3((unsigned)nl), dim3(64), ext_lds, st, d_ext, d_elist, d_qs,
                    d_text, es, d_best, d_plan, d_edir);
            HIPCHECK(hipGetLastError());
            KLAUNCH("k_extend_trace", (double)nl * 36.0 + (double)eops_total * 4.0, k_extend_trace, dim3(blocks(nl)),
                    dim3(256), 0, st, d_elist, nl, We, d_best, d_plan, d_edir, d_eops, d_ecnt);
            HIPCHECK(hipGetLastError());
        }
        s_plan = d_plan;
        s_eops = d_eops;
        s_ecnt = d_ecnt;
    }

    // ---- the chains: count, scan, write
    KLAUNCH("k_align_stitch", (double)nmember * 12.0 + (double)ops_total * 4.0, k_align_stitch, dim3(blocks(nchain, 64)),
            dim3(64), 0, st, d_moff, nchain, d_blk, d_gaps, d_ops, d_opcnt, s_plan, s_eops, s_ecnt,
            (const uint32_t *)nullptr, (uint32_t *)nullptr, d_nops, d_nm, d_neq, d_cols);
    HIPCHECK(hipGetLastError());
    exclusive_scan<uint32_t>(c, d_nops, d_coff, nchain + 1);
    uint32_t *mb = c.mailbox<uint32_t>(1);
    HIPCHECK(hipMemcpyAsync(mb, d_coff + C, 4, hipMemcpyDeviceToHost, st));
    scan_wait(st);   // (the uploads above read pageable arrays: they are done too)
    const int64_t ncigar = mb[0];
    if (ncigar < nchain || ncigar > ops_total + nmember + eops_total)
        fail(BWTMI_E_STATE, "align: %lld operations out of %lld chains", (long long)ncigar, (long long)nchain);
    c.slot[S_IDX1].ensure((size_t)ncigar * 4);
    uint32_t *d_cigar = c.slot[S_IDX1].as<uint32_t>();
    KLAUNCH("k_align_stitch", (double)nmember * 12.0 + (double)ops_total * 4.0 + (double)ncigar * 4.0, k_align_stitch,
            dim3(blocks(nchain, 64)), dim3(64), 0, st, d_moff, nchain, d_blk, d_gaps, d_ops, d_opcnt, s_plan, s_eops,
            s_ecnt, (const uint32_t *)d_coff, d_cigar, d_nops, d_nm, d_neq, d_cols);
    HIPCHECK(hipGetLastError());

    std::vector<uint32_t> coff(C + 1);
    out.cigar.resize((size_t)ncigar);
    out.nm.resize(C);
    out.n_eq.resize(C);
    out.cols.resize(C);
    HIPCHECK(hipMemcpyAsync(coff.data(), d_coff, (C + 1) * 4, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(out.nm.data(), d_nm, C * 4, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(out.n_eq.data(), d_neq, C * 4, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(out.cols.data(), d_cols, C * 4, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(out.cigar.data(), d_cigar, (size_t)ncigar * 4, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    out.cigar_off.assign(coff.begin(), coff.end());
}

}  // namespace

void index_align_chains(Ctx &c, DeviceIndex *ix, const uint8_t *qs, const int64_t *off, int64_t nq,
                        const int64_t *chain_off, const uint8_t *strand, const int64_t *member_off,
                        const int32_t *mq, const int64_t *mr, const int32_t *mlen, int64_t nchain, int64_t nmember,
                        const AlignParams &p, AlignResult &out) {
    align_run(c, ix, qs, off, nq, chain_off, strand, member_off, mq, mr, mlen, nchain, nmember, p, nullptr, out);
}

void index_align_extend(Ctx &c, DeviceIndex *ix, const uint8_t *qs, const int64_t *off, int64_t nq,
                        const int64_t *chain_off, const uint8_t *strand, const int64_t *member_off,
                        const int32_t *mq, const int64_t *mr, const int32_t *mlen, int64_t nchain, int64_t nmember,
                        const AlignParams &p, const ExtendParams &e, AlignResult &out) {
    align_run(c, ix, qs, off, nq, chain_off, strand, member_off, mq, mr, mlen, nchain, nmember, p, &e, out);
}

}  // namespace bwtmi
