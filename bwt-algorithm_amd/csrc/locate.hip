// locate.hip -- batched locate over a resident FM index: every occurrence of
// every pattern with at most k substitutions, on one or both strands
// (contract: include/bwtmi.h, bwtmi_index_locate_batch).
//
// Pigeonhole seed-and-verify.  The searched string Q (the pattern, or its
// reverse complement) is cut into k + 1 pieces; a window with <= k
// substitutions holds at least one piece exactly, so the exact occurrences of
// the pieces enumerate a superset of the hits:
//   host          piece table (pattern, strand, piece offset), Q bytes
//   k_loc_seed*   exact backward search per piece, interval left on the device
//                 (index.hip, the rank paths of index_backward_search)
//   scan          exclusive_scan<int64_t> of the widths; the total is the
//                 call's candidate count, read back once and held against the cap
//   k_loc_verify  one lane per candidate: SA row -> window start, compare the
//                 window with Q in the resident text, keep the candidate only
//                 when its piece is the first exact piece of the window (so a
//                 hit survives once, no dedup sort), wave-compacted output
//   sort          radix_sort_pairs32 over the (pattern, position, strand) key
//                 bits in use; keys are unique, so the order is deterministic
//   k_loc_unpack  keys -> positions / strands / per-pattern offsets
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "device.h"

namespace bwtmi {

namespace {

// info: m (11 bits) | piece offset in Q << 11 (11 bits) | piece index << 22 (2 bits) | strand << 24
struct LocPiece {
    int64_t qoff;   // where Q starts in the uploaded bytes
    int32_t pat;
    uint32_t info;
};
static_assert(kLocMaxPattern <= 1024 && kLocMaxMismatch <= 3, "LocPiece::info field widths");

inline unsigned blocks(int64_t n, int b = 256) { return (unsigned)((n + b - 1) / b); }

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
        int64_t lo = 0, hi = np;   // cum[lo] <= t < cum[hi]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (cum[mid] <= t) lo = mid;
            else hi = mid;
        }
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

}  // namespace

void index_locate_batch(Ctx &c, DeviceIndex *ix, const uint8_t *pats, const int64_t *off, int64_t npat,
                        int32_t max_mismatch, bool both_strands, int64_t max_candidates, LocateResult &out) {
    const int k = max_mismatch;
    if (k < 0 || k > kLocMaxMismatch) fail(BWTMI_E_ARG, "locate: max_mismatch %d outside 0..%d", k, kLocMaxMismatch);
    if (npat < 0) fail(BWTMI_E_ARG, "locate: negative pattern count");
    if (max_candidates <= 0) max_candidates = kLocDefaultCap;
    const int64_t n = index_n(ix);
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
        int strands = 1;
        if (both_strands) {
            rc.resize((size_t)m);
            for (int64_t i = 0; i < m; ++i) rc[(size_t)i] = comp_byte(pats[a + m - 1 - i]);
            if (std::memcmp(rc.data(), pats + a, (size_t)m) != 0) strands = 2;   // its own reverse complement: '+' only
        }
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

    // ---- seeds, widths -> offsets, the candidate count against the cap
    index_seed_search_device(c, ix, d_q, d_pstart, np, plen, d_row0, d_cum);
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
            d_pieces, d_q, index_text_device(ix), index_sa_device(ix), n, ttot, k, posbits, d_keys, d_vals, d_cursor);
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

}  // namespace bwtmi
