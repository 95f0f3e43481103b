// smem.hip -- batched SMEM seeding over a resident FM index: the super-maximal
// exact matches of every query, on one or both strands, with their occurrences
// (contract: include/bwtmi.h, bwtmi_index_smem_batch).
//
// One lane per (searched string, end e); the strings (a query, then its
// reverse complement where that is searched) lie back to back, so lane g is
// byte g, and a '-' string takes its ends descending: lane order is already
// (query, strand, qstart) order, and the compaction below keeps it.
//   host            string table, the strings' bytes
//   k_smem_ms*      l(e) and the SA interval of Q[e - l(e), e) per lane
//                   (index.hip, the rank paths of index_backward_search)
//   k_smem_flag     SMEM flag from l(e), l(e + 1) and min_len; l(e) and the
//                   width gated by max_occ, widened for the scans
//   scans           exclusive_scan<int64_t> of the three: SMEM index, work,
//                   position offset; the three totals are read back once and
//                   the position count held against the cap
//   k_smem_compact  flagged lanes -> the SMEM table, in lane order (no atomics)
//   k_smem_occ      one lane per reported position: (SMEM << posbits) | SA value
//   sort            radix_sort_pairs32 over the key bits in use
//   k_smem_unpack   keys -> positions
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "device.h"

namespace bwtmi {

namespace {

inline unsigned blocks(int64_t n, int b = 256) { return (unsigned)((n + b - 1) / b); }

inline uint8_t comp_byte(uint8_t ch) {   // the locate rule (locate.hip)
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
        const int m = (int)(s.info & 2047u);
        l = ell[g];
        if (l >= min_len) {
            if (e == m) f = 1;
            else f = ell[(s.info >> 11) & 1u ? g - 1 : g + 1] <= l;
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
    const int m = (int)(s.info & 2047u), l = ell[g];
    const bool minus = (s.info >> 11) & 1u;
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
    int64_t lo = 0, hi = nsmem;   // pos_off[lo] <= t < pos_off[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (pos_off[mid] <= t) lo = mid;
        else hi = mid;
    }
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

void index_smem_batch(Ctx &c, DeviceIndex *ix, const uint8_t *qs, const int64_t *off, int64_t nq, int32_t min_len,
                      bool both_strands, int64_t max_occ, int64_t max_positions, SmemResult &out) {
    if (nq < 0) fail(BWTMI_E_ARG, "smem: negative query count");
    if (min_len < 1) fail(BWTMI_E_ARG, "smem: min_len %d is below 1", min_len);
    if (max_occ <= 0) max_occ = kSmemDefaultMaxOcc;
    if (max_positions <= 0) max_positions = kLocDefaultCap;
    const int64_t n = index_n(ix);
    out.smem_off.assign((size_t)nq + 1, 0);
    out.qstart.clear();
    out.qend.clear();
    out.strand.clear();
    out.count.clear();
    out.pos_off.assign(1, 0);
    out.pos.clear();
    out.positions_total = out.work = 0;

    // ---- string table: Q, then revcomp(Q) where it is searched; string s is bytes [qoff, qoff + m)
    std::vector<uint8_t> qbytes;
    std::vector<SmemStr> strs;
    std::vector<int64_t> qlane((size_t)nq + 1, 0);
    std::vector<uint8_t> rc;
    double max_steps = 0;
    for (int64_t q = 0; q < nq; ++q) {
        const int64_t a = off[q], m = off[q + 1] - a;
        if (m <= 0) fail(BWTMI_E_ARG, "smem: query %lld is empty", (long long)q);
        if (m > kSmemMaxQuery)
            fail(BWTMI_E_ARG, "smem: query %lld has %lld bytes, more than the supported %lld", (long long)q,
                 (long long)m, (long long)kSmemMaxQuery);
        int strands = 1;
        if (both_strands) {
            rc.resize((size_t)m);
            for (int64_t i = 0; i < m; ++i) rc[(size_t)i] = comp_byte(qs[a + m - 1 - i]);
            if (std::memcmp(rc.data(), qs + a, (size_t)m) != 0) strands = 2;   // its own reverse complement: '+' only
        }
        qlane[(size_t)q] = (int64_t)qbytes.size();
        for (int s = 0; s < strands; ++s) {
            const uint8_t *src = s ? rc.data() : qs + a;
            strs.push_back({(int64_t)qbytes.size(), (int32_t)q, (uint32_t)m | (uint32_t)s << 11});
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

    // ---- matching statistics, flags, the three scans; their totals against the cap
    index_smem_ms_device(c, ix, d_q, d_str, ns, nl, max_steps, d_ell, d_row0, d_width);
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
    scan_wait(st);   // (the uploads above read pageable host vectors: they are done too)
    const int64_t nsmem = mb[0], npos = mb[2];
    out.work = mb[1];
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
                d_poff, nsmem, d_srow, index_sa_device(ix), n, npos, posbits, d_keys, d_vals);
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

}  // namespace bwtmi
