// search.hip -- everything that reads a built FM index (index.hip builds it):
// backward search (bwt.py:335-389), SA rows, batched locate with mismatches and
// batched SMEM seeding (contracts: include/bwtmi.h).
//
// An index is read through one of two rank paths, two types with the same
// members (n, start, step, and the SMEM search's wrap rule):
//   FM2View  the packed 2-bit blocks of ACGT* '$' texts
//   FMView   the byte BWT plus sampled Occ: every other text, BWTMI_FM_BYTES=1
// with_rank() chooses; the per-lane search and the three kernels built on the
// steps (k_bsearch, k_loc_seed, k_smem_ms) are templates over the path.
//
// Locate: pigeonhole seed-and-verify.  The searched string Q (the pattern, or
// its reverse complement) is cut into k + 1 pieces; a window with <= k
// substitutions holds at least one piece exactly, so the exact occurrences of
// the pieces enumerate a superset of the hits:
//   host          piece table (pattern, strand, piece offset), Q bytes
//   k_loc_seed    exact backward search per piece, interval left on the device
//   scan          exclusive_scan<int64_t> of the widths; the total is the
//                 call's candidate count, read back once and held against the cap
//   k_loc_verify  one lane per candidate: SA row -> window start, compare the
//                 window with Q in the resident text, keep the candidate only
//                 when its piece is the first exact piece of the window (so a
//                 hit survives once, no dedup sort), wave-compacted output
//   sort          radix_sort_pairs32 over the (pattern, position, strand) key
//                 bits in use; keys are unique, so the order is deterministic
//   k_loc_unpack  keys -> positions / strands / per-pattern offsets
//
// SMEM: one lane per (searched string, end e); the strings (a query, then its
// reverse complement where that is searched) lie back to back, so lane g is
// byte g, and a '-' string takes its ends descending: lane order is already
// (query, strand, qstart) order, and the compaction below keeps it.
//   host            string table, the strings' bytes
//   k_smem_ms       l(e) and the SA interval of Q[e - l(e), e) per lane
//   k_smem_flag     SMEM flag from l(e), l(e + 1) and min_len; l(e) and the
//                   width gated by max_occ, widened for the scans
//   scans           exclusive_scan<int64_t> of the three: SMEM index, work,
//                   position offset; the three totals are read back once and
//                   the position count held against the cap
//   k_smem_compact  flagged lanes -> the SMEM table, in lane order (no atomics)
//   k_smem_occ      one lane per reported position: (SMEM << posbits) | SA value
//   sort            radix_sort_pairs32 over the key bits in use
//   k_smem_unpack   keys -> positions
// Long reads (index_smem_long_batch, an index with its reverse index): the
// matching statistics come from k_smem_walk instead, one lane per searched
// string, which walks the string's SMEMs left to right -- rightwards in the
// reverse index, leftwards in the forward one -- and fills the same three
// per-lane arrays; everything from k_smem_flag on is shared.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include "device.h"

namespace bwtmi {

namespace {

constexpr int kLocMaxMismatch = 3;
constexpr int64_t kLocMaxPattern = 1024;
constexpr int64_t kLocDefaultCap = int64_t{1} << 27;
constexpr int64_t kSmemMaxQuery = 1024;
constexpr int64_t kSmemMaxLongQuery = int64_t{1} << 20;
constexpr int64_t kSmemDefaultMaxOcc = 1024;

// ---- packed FM rank for ACGT* '$' texts (bwt.py:335-357 semantics)
struct FM2View {
    static constexpr bool packed = true;
    const uint4 *blk;      // 2 x uint4 per block
    int64_t C[5], tot[5];  // codes A C G T $
    int64_t n, dollar;

    static __device__ __forceinline__ int code5(uint8_t ch) {
        switch (ch) {
            case 'A': return 0;
            case 'C': return 1;
            case 'G': return 2;
            case 'T': return 3;
            case '$': return 4;
            default: return -1;
        }
    }

    // occurrences of code c (0-3; 4 = '$') in bwt[0, i), 0 <= i <= n
    __device__ __forceinline__ int64_t rank2(int c, int64_t i) const {
        if (c == 4) return dollar < i ? 1 : 0;
        const int64_t b = i >> 6;
        const int r = (int)(i & 63);
        const uint4 h = blk[2 * b], p = blk[2 * b + 1];
        const uint32_t cnt = c == 0 ? h.x : c == 1 ? h.y : c == 2 ? h.z : h.w;
        const uint64_t lo = ((uint64_t)p.y << 32) | p.x, hi = ((uint64_t)p.w << 32) | p.z;
        const uint64_t m = ((c & 1) ? lo : ~lo) & ((c & 2) ? hi : ~hi);
        const uint64_t below = r ? (~0ull >> (64 - r)) : 0ull;
        int64_t x = (int64_t)cnt + __popcll(m & below);
        if (c == 0 && dollar >= 64 * b && dollar < i) --x;   // the '$' row reads as A in the planes
        return x;
    }

    // [sp, ep] of the one-symbol string ch; false when ch does not occur
    __device__ __forceinline__ bool start(uint8_t ch, int64_t &sp, int64_t &ep) const {
        const int c = code5(ch);
        if (c < 0 || tot[c] == 0) return false;
        sp = C[c];
        ep = sp + tot[c] - 1;
        return true;
    }

    // one step of the backward search (two 32-byte block loads and two
    // popcounts): [sp, ep] of a string X -> [sp, ep] of ch X; false (sp, ep as
    // they were) when ch X does not occur
    __device__ __forceinline__ bool step(uint8_t ch, int64_t &sp, int64_t &ep) const {
        const int c = code5(ch);
        if (c < 0 || tot[c] == 0) return false;
        const int64_t s = C[c] + rank2(c, sp), e = C[c] + rank2(c, ep + 1) - 1;
        if (s > e) return false;
        sp = s;
        ep = e;
        return true;
    }

    // the SMEM search's step: step() for an X that must not wrap round the end
    // of the text (`last` = last_byte(), read once per lane; unused here)
    __device__ __forceinline__ uint8_t last_byte(const uint8_t *) const { return 0; }
    __device__ __forceinline__ bool smem_step(uint8_t ch, uint8_t, int64_t &sp, int64_t &ep) const {
        // the text's one '$' is its last byte: '$' X (X not empty) occurs nowhere, and the
        // step would find it wrapped round the end of the text
        return ch != '$' && step(ch, sp, ep);
    }
};

// ---- byte BWT + sampled Occ (bwt.py:335-389)
struct FMView {
    static constexpr bool packed = false;
    const uint8_t *bwt;
    const int32_t *occ;
    const int64_t *C;
    const int64_t *tot;
    const uint8_t *row;
    int64_t n, olen;
    int32_t k;

    __device__ int64_t d_rank(uint8_t c, int64_t pos) const {
        if (pos <= 0) return 0;
        if (pos > n) pos = n;
        const int64_t ci = pos / k, cpos = ci * k;
        int64_t base = occ[(int64_t)row[c] * olen + ci];
        for (int64_t i = cpos; i < pos; ++i) base += bwt[i] == c;
        return base;
    }

    __device__ __forceinline__ bool start(uint8_t c, int64_t &sp, int64_t &ep) const {
        if (tot[c] == 0) return false;
        sp = C[c];
        ep = sp + tot[c] - 1;
        return true;
    }

    // one step over the byte Occ (FM2View::step's contract)
    __device__ __forceinline__ bool step(uint8_t c, int64_t &sp, int64_t &ep) const {
        if (tot[c] == 0) return false;
        const int64_t s = C[c] + d_rank(c, sp), e = C[c] + d_rank(c, ep + 1) - 1;
        if (s > e) return false;
        sp = s;
        ep = e;
        return true;
    }

    __device__ __forceinline__ uint8_t last_byte(const uint8_t *text) const { return text[n - 1]; }
    __device__ __forceinline__ bool smem_step(uint8_t b, uint8_t last, int64_t &sp, int64_t &ep) const {
        int64_t s2 = sp, e2 = ep;
        if (!step(b, s2, e2)) return false;
        // the first row of the text's last byte is the suffix made of that byte alone:
        // 'b X' (X not empty) found there wraps round the end of the text
        if (b == last && s2 == C[b] && ++s2 > e2) return false;
        sp = s2;
        ep = e2;
        return true;
    }
};

FM2View fm2_view(const DeviceIndex *ix) {
    FM2View g;
    g.blk = ix->fm2.as<uint4>();
    const char sym[5] = {'A', 'C', 'G', 'T', '$'};
    for (int q = 0; q < 5; ++q) {
        g.C[q] = ix->C[(uint8_t)sym[q]];
        g.tot[q] = ix->totals[(uint8_t)sym[q]];
    }
    g.n = ix->n;
    g.dollar = ix->dollar_row;
    return g;
}
// the byte-Occ view; its C / totals / row tables go up into the S_MISC3 slot
// (place 1: the tables of a second view that is live beside the first)
constexpr size_t kFmTabBytes = 256 * 8 * 2 + 256;
FMView fm_view(Ctx &c, const DeviceIndex *ix, int place = 0) {
    hipStream_t st = c.stream;
    c.slot[S_MISC3].ensure(2 * kFmTabBytes);
    int64_t *tabs = reinterpret_cast<int64_t *>(c.slot[S_MISC3].as<uint8_t>() + place * kFmTabBytes);
    HIPCHECK(hipMemcpyAsync(tabs, ix->C, 256 * 8, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(tabs + 256, ix->totals, 256 * 8, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(tabs + 512, ix->code_of, 256, hipMemcpyHostToDevice, st));
    FMView f;
    f.bwt = ix->bwt.as<uint8_t>();
    f.occ = ix->occ.as<int32_t>();
    f.C = tabs;
    f.tot = tabs + 256;
    f.row = (const uint8_t *)(tabs + 512);
    f.n = ix->n;
    f.olen = index_occ_len(ix);
    f.k = ix->occ_sample;
    return f;
}

// The one choice of rank path: launch(rank) with the packed rank where the
// index has it and BWTMI_FM_BYTES does not forbid it, else with the byte rank
// (whose tables then go up into S_MISC3).  `Rank::packed` names the kernel.
template <class Launch>
void with_rank(Ctx &c, const DeviceIndex *ix, Launch &&launch, int place = 0) {
    if (ix->has_fm2 && !knob(KN_FM_BYTES)) launch(fm2_view(ix));
    else launch(fm_view(c, ix, place));
}

inline uint8_t comp_byte(uint8_t ch) {
    switch (ch) {
        case 'A': return 'T';
        case 'T': return 'A';
        case 'C': return 'G';
        case 'G': return 'C';
        default: return ch;
    }
}

inline int bits_for(int64_t values) {   // bits that hold 0 .. values - 1
    int b = 1;
    while (b < 63 && (int64_t{1} << b) < values) ++b;
    return b;
}

// The strings searched for s[0, m): string 0 is s, string 1 its reverse
// complement, written to rc, when both strands are asked for and the two
// differ.  Returns their count.
inline int strand_strings(const uint8_t *s, int64_t m, bool both_strands, std::vector<uint8_t> &rc) {
    if (!both_strands) return 1;
    rc.resize((size_t)m);
    uint8_t *r = rc.data();
    for (int64_t i = 0; i < m; ++i) r[i] = comp_byte(s[m - 1 - i]);
    return std::memcmp(r, s, (size_t)m) != 0 ? 2 : 1;   // its own reverse complement: '+' only
}

// ---- exact backward search, one pattern per lane: the lane's search of
// pats[a, b) (shared by k_bsearch and the locate seed search, k_loc_seed)
template <class Rank>
__device__ __forceinline__ void bsearch_lane(const Rank &f, const uint8_t *__restrict__ pats, int64_t a, int64_t b,
                                             int64_t &sp, int64_t &ep) {
    sp = ep = -1;
    if (b == a) {
        sp = 0;
        ep = f.n - 1;
        return;
    }
    if (f.start(pats[b - 1], sp, ep))
        for (int64_t i = b - 2; i >= a; --i)
            if (!f.step(pats[i], sp, ep)) { sp = ep = -1; break; }
}

template <class Rank>
__global__ __launch_bounds__(256) void k_bsearch(Rank f, const uint8_t *__restrict__ pats,
                                                 const int64_t *__restrict__ off, int64_t np,
                                                 int64_t *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    int64_t sp, ep;
    bsearch_lane(f, pats, off[p], off[p + 1], sp, ep);
    out[2 * p] = sp;
    out[2 * p + 1] = ep;
}

// the locate seed search: the interval's first row and its width (0 = no
// occurrence) of every piece, left on the device
template <class Rank>
__global__ __launch_bounds__(256) void k_loc_seed(Rank f, const uint8_t *__restrict__ pats,
                                                  const int64_t *__restrict__ off, int64_t np,
                                                  int64_t *__restrict__ row0, int64_t *__restrict__ width) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    int64_t sp, ep;
    bsearch_lane(f, pats, off[p], off[p + 1], sp, ep);
    row0[p] = sp < 0 ? 0 : sp;
    width[p] = sp < 0 ? 0 : ep - sp + 1;
}

__global__ void k_sa_rows(const uint32_t *__restrict__ sa, const int64_t *__restrict__ rows, int64_t k,
                          int64_t *__restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < k) out[j] = (int64_t)sa[rows[j]];
}

// ---- locate
// info: m (11 bits) | piece offset in Q << 11 (11 bits) | piece index << 22 (2 bits) | strand << 24
struct LocPiece {
    int64_t qoff;   // where Q starts in the uploaded bytes
    int32_t pat;
    uint32_t info;
};
static_assert(kLocMaxPattern <= 1024 && kLocMaxMismatch <= 3, "LocPiece::info field widths");

// One lane per candidate t of [0, ttot): cum (np + 1 scanned widths, cum[np] =
// ttot) names its piece, row0 + the rank inside the interval its SA row.
// Neighbouring lanes share a piece, so the SA loads are coalesced; the text
// windows are gathers.  The loops below end on the lane's own values only; the
// one cross-lane value (the wave's survivors) is a ballot.
__global__ __launch_bounds__(256) void k_loc_verify(const int64_t *__restrict__ cum, int64_t np,
                                                    const int64_t *__restrict__ row0,
                                                    const LocPiece *__restrict__ pieces,
                                                    const uint8_t *__restrict__ q, const uint8_t *__restrict__ text,
                                                    const uint32_t *__restrict__ sa, int64_t n, int64_t ttot, int k,
                                                    int posbits, uint64_t *__restrict__ keys,
                                                    uint32_t *__restrict__ vals, unsigned long long *__restrict__ cursor) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    uint64_t key = 0;
    int d = 0;
    if (t < ttot) {
        const int64_t lo = owner_of(np, t, [&](int64_t i) { return cum[i]; });
        const LocPiece pc = pieces[lo];
        const int m = (int)(pc.info & 2047u), poff = (int)((pc.info >> 11) & 2047u);
        const int j = (int)((pc.info >> 22) & 3u);
        const uint64_t strand = (pc.info >> 24) & 1u;
        const int64_t row = row0[lo] + (t - cum[lo]);
        const int64_t start = row < n ? (int64_t)sa[row] - poff : -1;
        if (start >= 0 && start + m <= n) {
            const uint8_t *__restrict__ w = text + start, *__restrict__ qq = q + pc.qoff;
            keep = true;
            for (int jj = 0; jj <= k && keep; ++jj) {
                if (jj == j) continue;   // the seed: exact by construction
                const int a = jj * m / (k + 1), b = (jj + 1) * m / (k + 1);
                int cnt = 0;
                for (int i = a; i < b; ++i) {
                    const uint8_t tb = w[i];
                    if (tb != qq[i]) {
                        // '$' is never substituted; more than k mismatches: no hit
                        if (tb == '$' || d + ++cnt > k) {
                            keep = false;
                            break;
                        }
                    }
                }
                // an earlier exact piece reports this window
                if (jj < j && cnt == 0) keep = false;
                d += cnt;
            }
            key = ((uint64_t)(uint32_t)pc.pat << (posbits + 1)) | ((uint64_t)start << 1) | strand;
        }
    }
    const uint64_t bal = __ballot(keep);
    if (bal == 0) return;   // scalar
    const int lane = threadIdx.x & 63;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(cursor, (unsigned long long)__popcll(bal));
    base = __shfl(base, 0);
    if (keep) {
        const unsigned long long slot = base + (unsigned long long)__popcll(bal & ((1ull << lane) - 1ull));
        if (slot < (unsigned long long)ttot) {   // every candidate yields at most one survivor
            keys[slot] = key;
            vals[slot] = (uint32_t)d;
        }
    }
}

// sorted keys -> output columns; the first hit of a pattern also writes the
// offsets of the empty patterns before it, the last hit those after it
__global__ __launch_bounds__(256) void k_loc_unpack(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                    int64_t nh, int64_t npat, int posbits, int64_t *__restrict__ pos,
                                                    uint8_t *__restrict__ mm, uint8_t *__restrict__ strand,
                                                    int64_t *__restrict__ hit_off) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nh) return;
    const uint64_t key = keys[i];
    const int64_t pat = (int64_t)(key >> (posbits + 1));
    pos[i] = (int64_t)((key >> 1) & ((1ull << posbits) - 1ull));
    strand[i] = (uint8_t)(key & 1u);
    mm[i] = (uint8_t)vals[i];
    const int64_t prev = i ? (int64_t)(keys[i - 1] >> (posbits + 1)) : -1;
    for (int64_t p = prev + 1; p <= pat && p <= npat; ++p) hit_off[p] = i;
    if (i == nh - 1)
        for (int64_t p = pat + 1; p <= npat; ++p) hit_off[p] = nh;
}

// ---- SMEM
// one searched string (a query, or its reverse complement): its bytes start at
// qoff of the uploaded bytes, which is also its first lane
struct SmemStr {
    int64_t qoff;
    int32_t query;
    uint32_t info;   // m (24 bits) | strand << 24
};
constexpr uint32_t kSmemLenMask = (1u << 24) - 1u;
constexpr int kSmemStrandBit = 24;
static_assert(kSmemMaxQuery <= kSmemLenMask && kSmemMaxLongQuery <= kSmemLenMask, "SmemStr::info field widths");

// Lane g is byte g of the strings laid back to back: its string (str: ns
// entries ascending by qoff, str[0].qoff = 0) and its end e in 1..m.  A '+'
// string takes its ends ascending, a '-' string descending, so that lane order
// is (query, strand, qstart) order.
__device__ __forceinline__ int smem_lane(const SmemStr *__restrict__ str, int64_t ns, int64_t g, SmemStr &s) {
    s = str[owner_of(ns, g, [&](int64_t i) { return str[i].qoff; })];
    const int m = (int)(s.info & kSmemLenMask), t = (int)(g - s.qoff);
    return (s.info >> kSmemStrandBit) & 1u ? m - t : t + 1;
}

// Matching statistics, one lane per (searched string, end e).  The lane
// extends Q[e - 1] leftwards while the interval stays non-empty: ell = l(e),
// row0 / width = the SA interval of Q[e - l, e) (width 0 when l = 0).  The
// lanes of a wave are consecutive ends of one string: at step j they read
// consecutive bytes and their l differ by at most their distance.  The loop
// ends on the lane's own interval only.
template <class Rank>
__global__ __launch_bounds__(256) void k_smem_ms(Rank f, const uint8_t *__restrict__ text,
                                                 const uint8_t *__restrict__ q, const SmemStr *__restrict__ str,
                                                 int64_t ns, int64_t nl, int32_t *__restrict__ ell,
                                                 int64_t *__restrict__ row0, int64_t *__restrict__ width) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nl) return;
    SmemStr s;
    const int e = smem_lane(str, ns, g, s);
    const uint8_t *__restrict__ qq = q + s.qoff;
    int l = 0;
    int64_t sp = 0, ep = -1;
    const uint8_t last = f.last_byte(text);
    if (f.start(qq[e - 1], sp, ep)) {
        l = 1;
        for (int i = e - 2; i >= 0 && f.smem_step(qq[i], last, sp, ep); --i) ++l;
    }
    ell[g] = l;
    row0[g] = sp;
    width[g] = ep - sp + 1;
}

// Matching statistics of long strings, one lane per searched string t (an
// index with its reverse index r, over R = reverse(T[0, n-1)) + z, z = T[n-1]).
// The lane walks the string's SMEMs left to right.  From a start i:
//   F  extend Q[i, j) rightwards while it occurs: the backward search of
//      reverse(Q[i, j)) in r, one plain step per byte.  A step by z finds the
//      row that wraps in R exactly when the match so far ends T[0, n-1), the
//      legitimate "...z" match, and nothing follows z: the extension stops.
//      A string that starts at z has j = i + 1.
//   l(e) = e - i for every end e not yet written up to j, no search needed:
//      s(e) = e - l(e) never decreases, i = s(previous j + 1), Q[i, j) occurs.
//   B(j)    [i, j) is an SMEM when long enough: its SA interval from the
//      backward search of Q[i, j) in f (start and smem_step, as k_smem_ms),
//      skipped when j - i < min_len (k_smem_flag reads no width there).
//   B(j+1)  the next start s(j + 1) = j + 1 - l(j + 1): the backward search
//      from Q[j] in f, which is known to fail at Q[i] at the latest.
// It writes what k_smem_ms writes, at the lanes smem_lane defines: ell at every
// end, row0 / width at the ends j it visits with j - i >= min_len (elsewhere
// they are not read).  steps[t] = the rank steps taken, failing ones included.
// Every loop ends on the lane's own bytes and intervals only.
template <class RankF, class RankR>
__global__ __launch_bounds__(256) void k_smem_walk(RankF f, RankR r, const uint8_t *__restrict__ text,
                                                   const uint8_t *__restrict__ q, const SmemStr *__restrict__ str,
                                                   int64_t ns, int min_len, int32_t *__restrict__ ell,
                                                   int64_t *__restrict__ row0, int64_t *__restrict__ width,
                                                   int64_t *__restrict__ steps) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ns) return;
    const SmemStr s = str[t];
    const int m = (int)(s.info & kSmemLenMask);
    const bool minus = (s.info >> kSmemStrandBit) & 1u;
    const uint8_t *__restrict__ qq = q + s.qoff;
    const uint8_t z = text[f.n - 1], last = f.last_byte(text);
    // the lane of end e (smem_lane's rule): 0 <= . < m past qoff for e in 1..m
    auto at = [&](int e) { return s.qoff + (minus ? m - e : e - 1); };
    int64_t nstep = 0, sp = 0, ep = -1;
    int i = 0, done = 0;   // ends 1..done are written; done >= i - 1
    while (i < m) {
        int j = i;
        if (r.start(qq[i], sp, ep)) {
            j = i + 1;
            if (qq[i] != z)
                while (j < m) {
                    const uint8_t b = qq[j];
                    ++nstep;
                    if (!r.step(b, sp, ep)) break;
                    ++j;
                    if (b == z) break;
                }
        }
        if (j == i) {   // Q[i] occurs nowhere: l(i + 1) = 0 (and l(i) = 0 where Q[i - 1] does not either)
            for (int e = done + 1; e <= i + 1; ++e) ell[at(e)] = 0;
            done = ++i;
            continue;
        }
        for (int e = done + 1; e <= j; ++e) ell[at(e)] = e - i;
        done = j;
        if (j - i >= min_len) {
            f.start(qq[j - 1], sp, ep);
            for (int k = j - 2; k >= i; --k) {
                ++nstep;
                f.smem_step(qq[k], last, sp, ep);
            }
            row0[at(j)] = sp;
            width[at(j)] = ep - sp + 1;
        }
        if (j == m) break;
        int l = 0;
        if (f.start(qq[j], sp, ep)) {
            l = 1;
            for (int k = j - 1; k > i; --k) {   // (Q[i, j + 1) does not occur)
                ++nstep;
                if (!f.smem_step(qq[k], last, sp, ep)) break;
                ++l;
            }
        }
        i = j + 1 - l;
    }
    for (int e = done + 1; e <= m; ++e) ell[at(e)] = 0;   // (the last byte occurs nowhere)
    steps[t] = nstep;
}

// Lanes 0 .. nl; lane nl writes the scans' last word.  l(e + 1) is the next
// lane of a '+' string and the previous lane of a '-' string; the lane of
// e = m has none and flags on its own l.
__global__ __launch_bounds__(256) void k_smem_flag(const SmemStr *__restrict__ str, int64_t ns, int64_t nl,
                                                   const int32_t *__restrict__ ell,
                                                   const int64_t *__restrict__ width, int min_len, int64_t max_occ,
                                                   int64_t *__restrict__ flag, int64_t *__restrict__ ell64,
                                                   int64_t *__restrict__ gated) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g > nl) return;
    int64_t f = 0, l = 0, w = 0;
    if (g < nl) {
        SmemStr s;
        const int e = smem_lane(str, ns, g, s);
        const int m = (int)(s.info & kSmemLenMask);
        l = ell[g];
        if (l >= min_len) {
            if (e == m) f = 1;
            else f = ell[(s.info >> kSmemStrandBit) & 1u ? g - 1 : g + 1] <= l;
        }
        if (f) {
            w = width[g];
            if (w > max_occ) w = 0;
        }
    }
    flag[g] = f;
    ell64[g] = l;
    gated[g] = w;
}

// fscan / gscan: the scanned flags and gated widths (nl + 1 words each).  Lane
// g < nl holds SMEM fscan[g] when fscan[g + 1] differs; lanes 0 .. nq also
// write the queries' offsets (qlane[q] = the first lane of query q, qlane[nq] =
// nl), lane nl the last position offset.
__global__ __launch_bounds__(256) void k_smem_compact(const SmemStr *__restrict__ str, int64_t ns, int64_t nl,
                                                      const int32_t *__restrict__ ell,
                                                      const int64_t *__restrict__ row0,
                                                      const int64_t *__restrict__ width,
                                                      const int64_t *__restrict__ fscan,
                                                      const int64_t *__restrict__ gscan,
                                                      const int64_t *__restrict__ qlane, int64_t nq, int64_t nsmem,
                                                      int32_t *__restrict__ qstart, int32_t *__restrict__ qend,
                                                      uint8_t *__restrict__ strand, int64_t *__restrict__ count,
                                                      int64_t *__restrict__ srow, int64_t *__restrict__ pos_off,
                                                      int64_t *__restrict__ smem_off) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g > nl) return;
    if (g <= nq) smem_off[g] = fscan[qlane[g]];
    if (g == nl) {
        pos_off[nsmem] = gscan[nl];
        return;
    }
    const int64_t i = fscan[g];
    if (fscan[g + 1] == i || i >= nsmem) return;
    SmemStr s;
    const int e = smem_lane(str, ns, g, s);
    const int m = (int)(s.info & kSmemLenMask), l = ell[g];
    const bool minus = (s.info >> kSmemStrandBit) & 1u;
    qstart[i] = minus ? m - e : e - l;
    qend[i] = minus ? m - e + l : e;
    strand[i] = minus ? 1 : 0;
    count[i] = width[g];
    srow[i] = row0[g];
    pos_off[i] = gscan[g];
}

// One lane per reported position t of [0, npos): pos_off (nsmem + 1 words,
// pos_off[nsmem] = npos) names its SMEM, srow + the rank inside the interval
// its SA row.  Neighbouring lanes share an SMEM, so the SA loads coalesce.
__global__ __launch_bounds__(256) void k_smem_occ(const int64_t *__restrict__ pos_off, int64_t nsmem,
                                                  const int64_t *__restrict__ srow, const uint32_t *__restrict__ sa,
                                                  int64_t n, int64_t npos, int posbits, uint64_t *__restrict__ keys,
                                                  uint32_t *__restrict__ vals) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= npos) return;
    const int64_t lo = owner_of(nsmem, t, [&](int64_t i) { return pos_off[i]; });
    const int64_t row = srow[lo] + (t - pos_off[lo]);
    const uint64_t p = row >= 0 && row < n ? sa[row] : 0;
    keys[t] = ((uint64_t)lo << posbits) | p;
    vals[t] = 0;
}

__global__ __launch_bounds__(256) void k_smem_unpack(const uint64_t *__restrict__ keys, int64_t npos, int posbits,
                                                     int64_t *__restrict__ pos) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < npos) pos[t] = (int64_t)(keys[t] & ((1ull << posbits) - 1ull));
}

}  // namespace

void index_backward_search(Ctx &c, DeviceIndex *ix, const uint8_t *pats, const int64_t *off, int64_t npat,
                           int64_t *sp_ep) {
    if (npat <= 0) return;
    hipStream_t st = c.stream;
    const int64_t plen = off[npat];
    c.slot[S_MISC0].ensure((size_t)plen + 8);
    c.slot[S_MISC1].ensure((size_t)(npat + 1) * 8);
    c.slot[S_MISC2].ensure((size_t)npat * 16);
    if (plen) HIPCHECK(hipMemcpyAsync(c.slot[S_MISC0].p, pats, (size_t)plen, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(c.slot[S_MISC1].p, off, (size_t)(npat + 1) * 8, hipMemcpyHostToDevice, st));
    with_rank(c, ix, [&](const auto &f) {
        using Rank = std::decay_t<decltype(f)>;
        KLAUNCH(Rank::packed ? "k_bsearch2" : "k_bsearch", 0.0, k_bsearch<Rank>, dim3(blocks(npat)), dim3(256), 0, st, f,
                c.slot[S_MISC0].as<uint8_t>(), c.slot[S_MISC1].as<int64_t>(), npat, c.slot[S_MISC2].as<int64_t>());
    });
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(sp_ep, c.slot[S_MISC2].p, (size_t)npat * 16, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
}

// SA[rows[j]] for k rows (host arrays; every row < n)
void index_sa_rows(Ctx &c, const DeviceIndex *ix, const int64_t *rows, int64_t k, int64_t *out) {
    if (k <= 0) return;
    for (int64_t j = 0; j < k; ++j)
        if (rows[j] < 0 || rows[j] >= ix->n) fail(BWTMI_E_ARG, "SA row %lld out of range", (long long)rows[j]);
    hipStream_t st = c.stream;
    c.slot[S_MISC0].ensure((size_t)k * 8);
    c.slot[S_MISC1].ensure((size_t)k * 8);
    HIPCHECK(hipMemcpyAsync(c.slot[S_MISC0].p, rows, (size_t)k * 8, hipMemcpyHostToDevice, st));
    KLAUNCH("k_sa_rows", 0.0, k_sa_rows, dim3(blocks(k)), dim3(256), 0, st, ix->sa.as<uint32_t>(),
                       c.slot[S_MISC0].as<int64_t>(), k, c.slot[S_MISC1].as<int64_t>());
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(out, c.slot[S_MISC1].p, (size_t)k * 8, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
}

void index_locate_batch(Ctx &c, DeviceIndex *ix, const uint8_t *pats, const int64_t *off, int64_t npat,
                        int32_t max_mismatch, bool both_strands, int64_t max_candidates, LocateResult &out) {
    const int k = max_mismatch;
    if (k < 0 || k > kLocMaxMismatch) fail(BWTMI_E_ARG, "locate: max_mismatch %d outside 0..%d", k, kLocMaxMismatch);
    if (npat < 0) fail(BWTMI_E_ARG, "locate: negative pattern count");
    if (max_candidates <= 0) max_candidates = kLocDefaultCap;
    const int64_t n = ix->n;
    out.hit_off.assign((size_t)npat + 1, 0);
    out.pos.clear();
    out.mm.clear();
    out.strand.clear();
    out.candidates = 0;

    // ---- piece table: the Qs back to back, so piece g is bytes [pstart[g], pstart[g + 1])
    std::vector<uint8_t> qbytes;
    std::vector<int64_t> pstart;
    std::vector<LocPiece> pieces;
    std::vector<uint8_t> rc;
    for (int64_t p = 0; p < npat; ++p) {
        const int64_t a = off[p], m = off[p + 1] - a;
        if (m <= 0) fail(BWTMI_E_ARG, "locate: pattern %lld is empty", (long long)p);
        if (m < k + 1)
            fail(BWTMI_E_ARG, "locate: pattern %lld has %lld bytes, fewer than max_mismatch + 1 = %d", (long long)p,
                 (long long)m, k + 1);
        if (m > kLocMaxPattern)
            fail(BWTMI_E_ARG, "locate: pattern %lld has %lld bytes, more than the supported %lld", (long long)p,
                 (long long)m, (long long)kLocMaxPattern);
        const int strands = strand_strings(pats + a, m, both_strands, rc);
        for (int s = 0; s < strands; ++s) {
            const int64_t qoff = (int64_t)qbytes.size();
            const uint8_t *src = s ? rc.data() : pats + a;
            qbytes.insert(qbytes.end(), src, src + m);
            for (int j = 0; j <= k; ++j) {
                const int64_t po = j * m / (k + 1);
                pstart.push_back(qoff + po);
                pieces.push_back({qoff, (int32_t)p,
                                  (uint32_t)m | (uint32_t)po << 11 | (uint32_t)j << 22 | (uint32_t)s << 24});
            }
        }
    }
    const int64_t np = (int64_t)pieces.size(), plen = (int64_t)qbytes.size();
    if (np == 0 || n == 0) return;
    pstart.push_back(plen);
    const int posbits = bits_for(n), patbits = bits_for(npat);
    if (npat > INT32_MAX || posbits + patbits + 1 > 64)
        fail(BWTMI_E_ARG, "locate: %lld patterns over %lld bytes do not fit the 64-bit hit key", (long long)npat,
             (long long)n);

    hipStream_t st = c.stream;
    c.slot[S_MISC0].ensure((size_t)plen + 8);
    c.slot[S_MISC1].ensure((size_t)(np + 1) * 8);
    c.slot[S_MISC2].ensure((size_t)np * sizeof(LocPiece));
    c.slot[S_SCAN].ensure((size_t)np * 8);
    c.slot[S_FLAG].ensure((size_t)(np + 1) * 8);
    c.slot[S_COUNTS].ensure(64);
    uint8_t *d_q = c.slot[S_MISC0].as<uint8_t>();
    int64_t *d_pstart = c.slot[S_MISC1].as<int64_t>();
    LocPiece *d_pieces = c.slot[S_MISC2].as<LocPiece>();
    int64_t *d_row0 = c.slot[S_SCAN].as<int64_t>(), *d_cum = c.slot[S_FLAG].as<int64_t>();
    unsigned long long *d_cursor = c.slot[S_COUNTS].as<unsigned long long>();
    HIPCHECK(hipMemcpyAsync(d_q, qbytes.data(), (size_t)plen, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_pstart, pstart.data(), (size_t)(np + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_pieces, pieces.data(), (size_t)np * sizeof(LocPiece), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemsetAsync(d_cum + np, 0, 8, st));
    HIPCHECK(hipMemsetAsync(d_cursor, 0, 8, st));

    // ---- seeds (the rank paths of index_backward_search), widths -> offsets, the candidate
    // count against the cap
    with_rank(c, ix, [&](const auto &f) {
        using Rank = std::decay_t<decltype(f)>;
        // per piece: its bytes and ~2 rank blocks per byte (gathers), 3 words in / out
        KLAUNCH(Rank::packed ? "k_loc_seed2" : "k_loc_seed", (double)plen * 65.0 + (double)np * 32.0, k_loc_seed<Rank>,
                dim3(blocks(np)), dim3(256), 0, st, f, d_q, d_pstart, np, d_row0, d_cum);
    });
    HIPCHECK(hipGetLastError());
    exclusive_scan<int64_t>(c, d_cum, d_cum, np + 1);
    int64_t *mb = c.mailbox<int64_t>(2);
    HIPCHECK(hipMemcpyAsync(mb, d_cum + np, 8, hipMemcpyDeviceToHost, st));
    scan_wait(st);   // (the uploads above read pageable host vectors: they are done too)
    const int64_t ttot = mb[0];
    out.candidates = ttot;
    if (ttot > max_candidates)
        fail(BWTMI_E_NOMEM, "locate: %lld candidates exceed max_candidates = %lld (nothing was truncated)",
             (long long)ttot, (long long)max_candidates);
    if (ttot == 0) return;
    if (ttot >= (int64_t{1} << 32)) fail(BWTMI_E_NOMEM, "locate: %lld candidates exceed the sort's 2^32", (long long)ttot);

    // ---- verify + compact
    c.slot[S_CAND_K].ensure((size_t)ttot * 8);
    c.slot[S_CAND_V].ensure((size_t)ttot * 4);
    uint64_t *d_keys = c.slot[S_CAND_K].as<uint64_t>();
    uint32_t *d_vals = c.slot[S_CAND_V].as<uint32_t>();
    // per candidate: its SA row, one 64-byte line of text (a gather), the Q bytes from cache
    KLAUNCH("k_loc_verify", (double)ttot * 68.0, k_loc_verify, dim3(blocks(ttot)), dim3(256), 0, st, d_cum, np, d_row0,
            d_pieces, d_q, ix->text.as<uint8_t>(), ix->sa.as<uint32_t>(), n, ttot, k, posbits, d_keys, d_vals, d_cursor);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(mb + 1, d_cursor, 8, hipMemcpyDeviceToHost, st));
    scan_wait(st);
    const int64_t nh = mb[1];
    if (nh < 0 || nh > ttot) fail(BWTMI_E_STATE, "locate: %lld hits out of %lld candidates", (long long)nh, (long long)ttot);
    if (nh == 0) return;

    // ---- order, unpack, copy down once
    radix_sort_pairs32(c, d_keys, d_vals, nh, 0, posbits + patbits + 1);
    c.slot[S_HITS].ensure((size_t)nh * 8);
    c.slot[S_CAND_K2].ensure((size_t)nh);
    c.slot[S_CAND_V2].ensure((size_t)nh);
    c.slot[S_IDX0].ensure((size_t)(npat + 1) * 8);
    int64_t *d_pos = c.slot[S_HITS].as<int64_t>(), *d_hoff = c.slot[S_IDX0].as<int64_t>();
    uint8_t *d_mm = c.slot[S_CAND_K2].as<uint8_t>(), *d_strand = c.slot[S_CAND_V2].as<uint8_t>();
    KLAUNCH("k_loc_unpack", (double)nh * 22.0 + (double)npat * 8.0, k_loc_unpack, dim3(blocks(nh)), dim3(256), 0, st,
            d_keys, d_vals, nh, npat, posbits, d_pos, d_mm, d_strand, d_hoff);
    HIPCHECK(hipGetLastError());
    out.pos.resize((size_t)nh);
    out.mm.resize((size_t)nh);
    out.strand.resize((size_t)nh);
    HIPCHECK(hipMemcpyAsync(out.pos.data(), d_pos, (size_t)nh * 8, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(out.mm.data(), d_mm, (size_t)nh, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(out.strand.data(), d_strand, (size_t)nh, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(out.hit_off.data(), d_hoff, (size_t)(npat + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
}

namespace {

// the two SMEM entries: long_entry = matching statistics by k_smem_walk over the
// index's reverse index (queries up to kSmemMaxLongQuery), else by k_smem_ms
void smem_batch(Ctx &c, DeviceIndex *ix, const uint8_t *qs, const int64_t *off, int64_t nq, int32_t min_len,
                bool both_strands, int64_t max_occ, int64_t max_positions, bool long_entry, SmemResult &out) {
    const int64_t max_query = long_entry ? kSmemMaxLongQuery : kSmemMaxQuery;
    if (nq < 0) fail(BWTMI_E_ARG, "smem: negative query count");
    if (min_len < 1) fail(BWTMI_E_ARG, "smem: min_len %d is below 1", min_len);
    if (max_occ <= 0) max_occ = kSmemDefaultMaxOcc;
    if (max_positions <= 0) max_positions = kLocDefaultCap;
    const int64_t n = ix->n;
    out.smem_off.assign((size_t)nq + 1, 0);
    out.qstart.clear();
    out.qend.clear();
    out.strand.clear();
    out.count.clear();
    out.pos_off.assign(1, 0);
    out.pos.clear();
    out.positions_total = out.work = out.steps = 0;
    if (long_entry && !ix->rev)
        fail(BWTMI_E_STATE, "smem: the index has no reverse index (build it with BWTMI_INDEX_REVERSE)");

    // ---- string table: Q, then revcomp(Q) where it is searched; string s is bytes [qoff, qoff + m)
    std::vector<uint8_t> qbytes;
    std::vector<SmemStr> strs;
    std::vector<int64_t> qlane((size_t)nq + 1, 0);
    std::vector<uint8_t> rc;
    double max_steps = 0;
    for (int64_t q = 0; q < nq; ++q) {
        const int64_t a = off[q], m = off[q + 1] - a;
        if (m <= 0) fail(BWTMI_E_ARG, "smem: query %lld is empty", (long long)q);
        if (m > max_query)
            fail(BWTMI_E_ARG, "smem: query %lld has %lld bytes, more than the supported %lld", (long long)q,
                 (long long)m, (long long)max_query);
        qlane[(size_t)q] = (int64_t)qbytes.size();
        const int strands = strand_strings(qs + a, m, both_strands, rc);
        for (int s = 0; s < strands; ++s) {
            const uint8_t *src = s ? rc.data() : qs + a;
            strs.push_back({(int64_t)qbytes.size(), (int32_t)q, (uint32_t)m | (uint32_t)s << kSmemStrandBit});
            qbytes.insert(qbytes.end(), src, src + m);
            max_steps += 0.5 * (double)m * (double)(m + 1);
        }
    }
    const int64_t ns = (int64_t)strs.size(), nl = (int64_t)qbytes.size();
    qlane[(size_t)nq] = nl;
    if (nl == 0 || n == 0) return;
    const int posbits = bits_for(n);
    if (nq > INT32_MAX || posbits + bits_for(nl) > 64)
        fail(BWTMI_E_ARG, "smem: %lld query bytes over %lld text bytes do not fit the 64-bit position key",
             (long long)nl, (long long)n);

    hipStream_t st = c.stream;
    c.slot[S_MISC0].ensure((size_t)nl + 8);
    c.slot[S_MISC1].ensure((size_t)(nq + 1) * 8);
    c.slot[S_MISC2].ensure((size_t)ns * sizeof(SmemStr));
    c.slot[S_CAND_V].ensure((size_t)nl * 4);
    c.slot[S_SCAN].ensure((size_t)nl * 8);
    c.slot[S_FLAG].ensure((size_t)nl * 8);
    c.slot[S_IDX0].ensure((size_t)(nl + 1) * 8);
    c.slot[S_IDX1].ensure((size_t)(nl + 1) * 8);
    c.slot[S_IDX2].ensure((size_t)(nl + 1) * 8);
    uint8_t *d_q = c.slot[S_MISC0].as<uint8_t>();
    int64_t *d_qlane = c.slot[S_MISC1].as<int64_t>();
    SmemStr *d_str = c.slot[S_MISC2].as<SmemStr>();
    int32_t *d_ell = c.slot[S_CAND_V].as<int32_t>();
    int64_t *d_row0 = c.slot[S_SCAN].as<int64_t>(), *d_width = c.slot[S_FLAG].as<int64_t>();
    int64_t *d_fscan = c.slot[S_IDX0].as<int64_t>(), *d_wscan = c.slot[S_IDX1].as<int64_t>();
    int64_t *d_gscan = c.slot[S_IDX2].as<int64_t>();
    HIPCHECK(hipMemcpyAsync(d_q, qbytes.data(), (size_t)nl, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_qlane, qlane.data(), (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_str, strs.data(), (size_t)ns * sizeof(SmemStr), hipMemcpyHostToDevice, st));

    // ---- matching statistics (the rank paths of index_backward_search), flags, the three
    // scans; their totals against the cap
    int64_t *d_steps = nullptr;
    if (long_entry) {
        c.slot[S_IDX10].ensure((size_t)ns * 8);
        d_steps = c.slot[S_IDX10].as<int64_t>();
        with_rank(c, ix, [&](const auto &f) {
            with_rank(c, ix->rev, [&](const auto &r) {
                using RankF = std::decay_t<decltype(f)>;
                using RankR = std::decay_t<decltype(r)>;
                // a model: a string that matches in a few long stretches takes ~3 steps
                // per byte (F, B(j), B(j + 1)), a byte and two 32-byte rank blocks each,
                // and writes l(e) for every end; the steps really taken are `steps`.
                // 64 lanes a workgroup: a lane is a whole string, so the strings spread
                // over as many CUs as there are waves
                KLAUNCH(RankF::packed ? "k_smem_walk2" : "k_smem_walk", (double)nl * (3.0 * 65.0 + 4.0) + (double)ns * 28.0,
                        (k_smem_walk<RankF, RankR>), dim3(blocks(ns, 64)), dim3(64), 0, st, f, r, ix->text.as<uint8_t>(),
                        d_q, d_str, ns, (int)min_len, d_ell, d_row0, d_width, d_steps);
            }, 1);
        });
    } else with_rank(c, ix, [&](const auto &f) {
        using Rank = std::decay_t<decltype(f)>;
        // a model, not a count: l(e) is not known before the launch, so every lane
        // is taken to run its e steps (max_steps = their sum; a read copied from the
        // text does), a byte and two 32-byte rank blocks each, 20 bytes out.  The
        // steps really taken are the call's `work`.
        KLAUNCH(Rank::packed ? "k_smem_ms2" : "k_smem_ms", max_steps * 65.0 + (double)nl * 20.0, k_smem_ms<Rank>,
                dim3(blocks(nl)), dim3(256), 0, st, f, ix->text.as<uint8_t>(), d_q, d_str, ns, nl, d_ell, d_row0,
                d_width);
    });
    HIPCHECK(hipGetLastError());
    KLAUNCH("k_smem_flag", (double)nl * 36.0, k_smem_flag, dim3(blocks(nl + 1)), dim3(256), 0, st, d_str, ns, nl, d_ell,
            d_width, (int)min_len, max_occ, d_fscan, d_wscan, d_gscan);
    HIPCHECK(hipGetLastError());
    exclusive_scan<int64_t>(c, d_fscan, d_fscan, nl + 1);
    exclusive_scan<int64_t>(c, d_wscan, d_wscan, nl + 1);
    exclusive_scan<int64_t>(c, d_gscan, d_gscan, nl + 1);
    int64_t *mb = c.mailbox<int64_t>(3);
    HIPCHECK(hipMemcpyAsync(mb, d_fscan + nl, 8, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(mb + 1, d_wscan + nl, 8, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(mb + 2, d_gscan + nl, 8, hipMemcpyDeviceToHost, st));
    std::vector<int64_t> lane_steps;
    if (long_entry) {
        lane_steps.resize((size_t)ns);
        HIPCHECK(hipMemcpyAsync(lane_steps.data(), d_steps, (size_t)ns * 8, hipMemcpyDeviceToHost, st));
    }
    scan_wait(st);   // (the uploads above read pageable host vectors: they are done too)
    const int64_t nsmem = mb[0], npos = mb[2];
    out.work = mb[1];
    for (int64_t v : lane_steps) out.steps += v;
    out.positions_total = npos;
    if (nsmem < 0 || nsmem > nl || npos < 0)
        fail(BWTMI_E_STATE, "smem: %lld SMEMs with %lld positions out of %lld lanes", (long long)nsmem, (long long)npos,
             (long long)nl);
    if (npos > max_positions)
        fail(BWTMI_E_NOMEM, "smem: %lld positions exceed max_positions = %lld (nothing was truncated)", (long long)npos,
             (long long)max_positions);
    if (npos >= (int64_t{1} << 32)) fail(BWTMI_E_NOMEM, "smem: %lld positions exceed the sort's 2^32", (long long)npos);
    if (nsmem == 0) return;

    // ---- the SMEM table in lane order
    c.slot[S_IDX3].ensure((size_t)nsmem * 4);
    c.slot[S_IDX4].ensure((size_t)nsmem * 4);
    c.slot[S_IDX5].ensure((size_t)nsmem);
    c.slot[S_IDX6].ensure((size_t)nsmem * 8);
    c.slot[S_IDX7].ensure((size_t)nsmem * 8);
    c.slot[S_IDX8].ensure((size_t)(nsmem + 1) * 8);
    c.slot[S_IDX9].ensure((size_t)(nq + 1) * 8);
    int32_t *d_qstart = c.slot[S_IDX3].as<int32_t>(), *d_qend = c.slot[S_IDX4].as<int32_t>();
    uint8_t *d_strand = c.slot[S_IDX5].as<uint8_t>();
    int64_t *d_count = c.slot[S_IDX6].as<int64_t>(), *d_srow = c.slot[S_IDX7].as<int64_t>();
    int64_t *d_poff = c.slot[S_IDX8].as<int64_t>(), *d_soff = c.slot[S_IDX9].as<int64_t>();
    KLAUNCH("k_smem_compact", (double)nl * 16.0 + (double)nsmem * 53.0 + (double)nq * 16.0, k_smem_compact,
            dim3(blocks(nl + 1)), dim3(256), 0, st, d_str, ns, nl, d_ell, d_row0, d_width, d_fscan, d_gscan, d_qlane, nq,
            nsmem, d_qstart, d_qend, d_strand, d_count, d_srow, d_poff, d_soff);
    HIPCHECK(hipGetLastError());

    // ---- the occurrences, ascending inside every SMEM
    if (npos > 0) {
        c.slot[S_CAND_K].ensure((size_t)npos * 8);
        c.slot[S_CAND_V2].ensure((size_t)npos * 4);
        c.slot[S_HITS].ensure((size_t)npos * 8);
        uint64_t *d_keys = c.slot[S_CAND_K].as<uint64_t>();
        uint32_t *d_vals = c.slot[S_CAND_V2].as<uint32_t>();
        int64_t *d_pos = c.slot[S_HITS].as<int64_t>();
        KLAUNCH("k_smem_occ", (double)npos * 16.0 + (double)nsmem * 16.0, k_smem_occ, dim3(blocks(npos)), dim3(256), 0, st,
                d_poff, nsmem, d_srow, ix->sa.as<uint32_t>(), n, npos, posbits, d_keys, d_vals);
        HIPCHECK(hipGetLastError());
        radix_sort_pairs32(c, d_keys, d_vals, npos, 0, posbits + bits_for(nsmem));
        KLAUNCH("k_smem_unpack", (double)npos * 16.0, k_smem_unpack, dim3(blocks(npos)), dim3(256), 0, st, d_keys, npos,
                posbits, d_pos);
        HIPCHECK(hipGetLastError());
        out.pos.resize((size_t)npos);
        HIPCHECK(hipMemcpyAsync(out.pos.data(), d_pos, (size_t)npos * 8, hipMemcpyDeviceToHost, st));
    }
    out.qstart.resize((size_t)nsmem);
    out.qend.resize((size_t)nsmem);
    out.strand.resize((size_t)nsmem);
    out.count.resize((size_t)nsmem);
    out.pos_off.resize((size_t)nsmem + 1);
    HIPCHECK(hipMemcpyAsync(out.qstart.data(), d_qstart, (size_t)nsmem * 4, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(out.qend.data(), d_qend, (size_t)nsmem * 4, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(out.strand.data(), d_strand, (size_t)nsmem, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(out.count.data(), d_count, (size_t)nsmem * 8, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(out.pos_off.data(), d_poff, (size_t)(nsmem + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(out.smem_off.data(), d_soff, (size_t)(nq + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
}

}  // namespace

void index_smem_batch(Ctx &c, DeviceIndex *ix, const uint8_t *qs, const int64_t *off, int64_t nq, int32_t min_len,
                      bool both_strands, int64_t max_occ, int64_t max_positions, SmemResult &out) {
    smem_batch(c, ix, qs, off, nq, min_len, both_strands, max_occ, max_positions, false, out);
}

void index_smem_long_batch(Ctx &c, DeviceIndex *ix, const uint8_t *qs, const int64_t *off, int64_t nq,
                           int32_t min_len, bool both_strands, int64_t max_occ, int64_t max_positions,
                           SmemResult &out) {
    smem_batch(c, ix, qs, off, nq, min_len, both_strands, max_occ, max_positions, true, out);
}

}  // namespace bwtmi
