// select.hip -- primary / secondary, MAPQ and pruning of a read's chains on the
// device (contract: include/bwtmi.h, bwtmi_select_chains).
//
// Chains (score, qstart, qend) arrive grouped (a group = one read, its chains of
// both strands and of every contig); a group's chains lie back to back in the
// input, and the group of a chain is always an upper-bound search of chain_off
// (owner_of), never a stored column.
//   k_select_keys    key = (group << sbits) | (max_score - score), value = the input
//                    index; sbits holds 0 .. max_score
//   sort             radix_sort_pairs32 over the key bits in use: stable, so the
//                    rank order (score descending, input index ascending)
//   k_select_parent  one wave per group, its chains in rank order; the 64 lanes
//                    test the primaries found so far 64 at a time, in list order,
//                    and a ballot's first set bit is the parent.  The list lives
//                    in LDS up to kSelLds primaries and past that in the group's
//                    own range of a global scratch column.  A last pass over the
//                    list writes the primaries' sub and MAPQ.
// Results land at the chain's input index: no output order depends on an atomic.
// (Two atomics per group sum the primaries and the kept chains, statistics.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device.h"

namespace bwtmi {

namespace {

constexpr int kSelLds = 256;   // primaries of a group held in LDS (5 KiB a wave); a multiple of 64

inline int select_bits_for(int64_t values) {   // bits that hold 0 .. values - 1
    int b = 1;
    while (b < 63 && (int64_t{1} << b) < values) ++b;
    return b;
}

__global__ __launch_bounds__(256) void k_select_keys(const int64_t *__restrict__ chain_off, int64_t ng,
                                                     const int32_t *__restrict__ score, int64_t nc, int32_t max_score,
                                                     int sbits, uint64_t *__restrict__ keys,
                                                     uint32_t *__restrict__ vals) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nc) return;
    const uint64_t g = (uint64_t)owner_of(ng, t, [&](int64_t i) { return chain_off[i]; });
    keys[t] = g << sbits | (uint64_t)(max_score - score[t]);
    vals[t] = (uint32_t)t;
}

// a primary of the list: its interval, its index relative to the group's first
// chain, its score and its best secondary's (0: none yet)
struct SelList {
    int32_t *qs, *qe, *idx, *score, *sub;
};

__device__ __forceinline__ int32_t select_mapq(int32_t s1, int32_t sub, int32_t full) {
    return (int32_t)((int64_t)60 * (s1 - sub) * min(s1, full) / ((int64_t)s1 * full));
}

// One workgroup of one wave per group.  Every loop bound and exit is a scalar
// (Guard): the group's range comes from blockIdx, the chain's own
// fields from wave-uniform addresses, the window count from the scalar list
// length, the hit from a ballot; no lane leaves a loop on its own value.  List
// entry j lives in LDS for j < kSelLds and at gl.*[a0 + j] past that: a group of
// n chains has at most n primaries, so its own range [a0, a0 + n) of the scratch
// columns holds them.  kSelLds is a multiple of 64, so a window is read from one
// of the two.  Lane 0 writes the list; the barrier that ends a chain's step
// orders its stores before the next chain's loads.
__global__ __launch_bounds__(64) void k_select_parent(const int64_t *__restrict__ chain_off,
                                                      const uint32_t *__restrict__ rank,
                                                      const int32_t *__restrict__ score,
                                                      const int32_t *__restrict__ qstart,
                                                      const int32_t *__restrict__ qend, int32_t mask, int32_t pri_ratio,
                                                      int32_t best_n, int32_t full, SelList gl,
                                                      int32_t *__restrict__ parent, int32_t *__restrict__ sub,
                                                      uint8_t *__restrict__ mapq, uint8_t *__restrict__ keep,
                                                      unsigned long long *__restrict__ counts) {
    __shared__ int32_t l_qs[kSelLds], l_qe[kSelLds], l_idx[kSelLds], l_score[kSelLds], l_sub[kSelLds];
    const int lane = (int)threadIdx.x;
    const int64_t a0 = chain_off[blockIdx.x];
    const int32_t n = (int32_t)(chain_off[blockIdx.x + 1] - a0);
    int32_t np = 0, nsec = 0;   // primaries found, secondaries kept
    for (int32_t t = 0; t < n; ++t) {
        const uint32_t c = __builtin_amdgcn_readfirstlane(rank[a0 + t]);
        const int32_t sc = __builtin_amdgcn_readfirstlane(score[c]);
        const int32_t cs = __builtin_amdgcn_readfirstlane(qstart[c]);
        const int32_t ce = __builtin_amdgcn_readfirstlane(qend[c]);
        int32_t hit = -1;
        for (int32_t w = 0; w < np; w += 64) {
            const int32_t j = w + lane;
            bool ok = false;
            if (j < np) {
                const int32_t ps = w < kSelLds ? l_qs[j] : gl.qs[a0 + j];
                const int32_t pe = w < kSelLds ? l_qe[j] : gl.qe[a0 + j];
                const int32_t ov = max(0, min(ce, pe) - max(cs, ps));
                ok = (int64_t)ov * 100 >= (int64_t)mask * min(ce - cs, pe - ps);
            }
            const unsigned long long b = __ballot(ok);
            if (b != 0) {
                hit = w + __ffsll(b) - 1;   // the first in list order
                break;
            }
        }
        const int32_t rel = (int32_t)((int64_t)c - a0);
        if (hit >= 0) {
            const bool lds = hit < kSelLds;
            const int32_t pidx = lds ? l_idx[hit] : gl.idx[a0 + hit];
            const int32_t pscore = lds ? l_score[hit] : gl.score[a0 + hit];
            const int32_t psub = lds ? l_sub[hit] : gl.sub[a0 + hit];
            const bool kept = (int64_t)sc * 100 >= (int64_t)pri_ratio * pscore && nsec < best_n;
            nsec += kept ? 1 : 0;
            if (lane == 0) {
                parent[c] = pidx;
                sub[c] = 0;
                mapq[c] = 0;
                keep[c] = kept ? 1 : 0;
                if (psub == 0) {   // the first secondary in rank order is the best
                    if (lds) l_sub[hit] = sc;
                    else gl.sub[a0 + hit] = sc;
                }
            }
        } else {
            if (lane == 0) {
                if (np < kSelLds) {
                    l_qs[np] = cs;
                    l_qe[np] = ce;
                    l_idx[np] = rel;
                    l_score[np] = sc;
                    l_sub[np] = 0;
                } else {
                    gl.qs[a0 + np] = cs;
                    gl.qe[a0 + np] = ce;
                    gl.idx[a0 + np] = rel;
                    gl.score[a0 + np] = sc;
                    gl.sub[a0 + np] = 0;
                }
                parent[c] = rel;
                keep[c] = 1;
            }
            ++np;
        }
        __syncthreads();   // one wave: lane 0's list stores before the next chain's loads
    }
    for (int32_t w = 0; w < np; w += 64) {
        const int32_t j = w + lane;
        if (j < np) {
            const bool lds = w < kSelLds;
            const int32_t pidx = lds ? l_idx[j] : gl.idx[a0 + j];
            const int32_t s1 = lds ? l_score[j] : gl.score[a0 + j];
            const int32_t sb = lds ? l_sub[j] : gl.sub[a0 + j];
            sub[a0 + pidx] = sb;
            mapq[a0 + pidx] = (uint8_t)select_mapq(s1, sb, full);
        }
    }
    if (lane == 0 && np) {
        atomicAdd(counts, (unsigned long long)np);
        atomicAdd(counts + 1, (unsigned long long)(np + nsec));
    }
}

// carves one slot into arrays (256-byte aligned)
struct SelectArena {
    size_t used = 0;
    uint8_t *base = nullptr;
    size_t take(size_t bytes) {
        const size_t at = used;
        used += (bytes + 255) & ~size_t{255};
        return at;
    }
    template <class T> T *at(size_t off) const { return reinterpret_cast<T *>(base + off); }
};

}  // namespace

void select_chains_device(Ctx &c, const int64_t *chain_off, int64_t ng, const int32_t *score, const int32_t *qstart,
                          const int32_t *qend, int32_t max_score, const SelectParams &p, SelectResult &out) {
    out = SelectResult{};
    const int64_t nc = ng > 0 ? chain_off[ng] : 0;
    if (nc == 0) return;
    if (nc >= (int64_t{1} << 31) || ng >= (int64_t{1} << 31))
        fail(BWTMI_E_NOMEM, "select: %lld chains in %lld groups exceed the 2^31 the selection indexes", (long long)nc,
             (long long)ng);
    const int sbits = select_bits_for((int64_t)max_score + 1), gbits = select_bits_for(ng);

    // ---- one slot, carved
    SelectArena ar;
    const size_t N = (size_t)nc;
    const size_t o_coff = ar.take((size_t)(ng + 1) * 8), o_score = ar.take(N * 4), o_qs = ar.take(N * 4), o_qe = ar.take(N * 4);
    const size_t o_keys = ar.take(N * 8), o_rank = ar.take(N * 4);
    const size_t o_lqs = ar.take(N * 4), o_lqe = ar.take(N * 4), o_lidx = ar.take(N * 4), o_lsc = ar.take(N * 4);
    const size_t o_lsub = ar.take(N * 4);
    const size_t o_parent = ar.take(N * 4), o_sub = ar.take(N * 4), o_mapq = ar.take(N), o_keep = ar.take(N);
    const size_t o_counts = ar.take(16);
    c.slot[S_IDX0].ensure(ar.used);
    ar.base = c.slot[S_IDX0].as<uint8_t>();
    int64_t *d_coff = ar.at<int64_t>(o_coff);
    int32_t *d_score = ar.at<int32_t>(o_score), *d_qs = ar.at<int32_t>(o_qs), *d_qe = ar.at<int32_t>(o_qe);
    uint64_t *d_keys = ar.at<uint64_t>(o_keys);
    uint32_t *d_rank = ar.at<uint32_t>(o_rank);
    const SelList gl{ar.at<int32_t>(o_lqs), ar.at<int32_t>(o_lqe), ar.at<int32_t>(o_lidx), ar.at<int32_t>(o_lsc),
                     ar.at<int32_t>(o_lsub)};
    int32_t *d_parent = ar.at<int32_t>(o_parent), *d_sub = ar.at<int32_t>(o_sub);
    uint8_t *d_mapq = ar.at<uint8_t>(o_mapq), *d_keep = ar.at<uint8_t>(o_keep);
    auto *d_counts = ar.at<unsigned long long>(o_counts);

    hipStream_t st = c.stream;
    // timed like a kernel (statistics name select_upload): what handing the chains' rows back to the device costs
    c.kbegin("select_upload", (double)nc * 12.0 + (double)(ng + 1) * 8.0);
    HIPCHECK(hipMemcpyAsync(d_coff, chain_off, (size_t)(ng + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_score, score, N * 4, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_qs, qstart, N * 4, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_qe, qend, N * 4, hipMemcpyHostToDevice, st));
    c.kend();
    HIPCHECK(hipMemsetAsync(d_counts, 0, 16, st));

    // ---- the contract's rank: (group, score descending), ties in input order
    KLAUNCH("k_select_keys", (double)nc * 16.0, k_select_keys, dim3(blocks(nc)), dim3(256), 0, st, d_coff, ng, d_score, nc,
            max_score, sbits, d_keys, d_rank);
    HIPCHECK(hipGetLastError());
    radix_sort_pairs32(c, d_keys, d_rank, nc, 0, sbits + gbits);

    // ---- parent, keep, mapq (bytes: the rank and the chain's 12 in, 10 out; the list stays in LDS or cache)
    KLAUNCH("k_select_parent", (double)nc * 26.0, k_select_parent, dim3((unsigned)ng), dim3(64), 0, st, d_coff, d_rank,
            d_score, d_qs, d_qe, p.mask, p.pri_ratio, p.best_n, p.full, gl, d_parent, d_sub, d_mapq, d_keep, d_counts);
    HIPCHECK(hipGetLastError());

    out.parent.resize(N);
    out.sub.resize(N);
    out.mapq.resize(N);
    out.keep.resize(N);
    unsigned long long *mb = c.mailbox<unsigned long long>(2);
    HIPCHECK(hipMemcpyAsync(mb, d_counts, 16, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(out.parent.data(), d_parent, N * 4, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(out.sub.data(), d_sub, N * 4, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(out.mapq.data(), d_mapq, N, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(out.keep.data(), d_keep, N, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    out.n_primary = (int64_t)mb[0];
    out.n_kept = (int64_t)mb[1];
    if (out.n_primary > nc || out.n_kept > nc || out.n_primary > out.n_kept)
        fail(BWTMI_E_STATE, "select: %lld primaries and %lld kept out of %lld chains", (long long)out.n_primary,
             (long long)out.n_kept, (long long)nc);
}

}  // namespace bwtmi
