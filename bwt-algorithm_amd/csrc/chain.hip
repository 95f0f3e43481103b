// chain.hip -- colinear chaining of anchors on the device, and the read mapper
// built on it (contracts: include/bwtmi.h, bwtmi_chain_anchors and
// bwtmi_index_map_batch).
//
// Anchors (q, r, len) arrive grouped (a group = one searched string); a group's
// anchors lie back to back in the input, and every stage below keeps a group in
// its input range [group_off[g], group_off[g + 1]), so the group of an element is
// always an upper-bound search of group_off (owner_of), never a stored column.
//   k_chain_keys    key = (re << qbits) | qe, value = the input index
//   sort            radix_sort_pairs32 over the key bits in use, then (more than
//                   one group) k_chain_gkeys + radix_sort_pairs_k32 by group: two
//                   stable sorts, since group, re and qe can exceed 64 bits
//   k_chain_gather  qe, re, len in sorted order
//   k_chain_dp      one wave per group, its anchors in sequence; the 64 lanes take
//                   the predecessor window 64 at a time, (score << 32) | j packed
//                   so that the wave maximum is the contract's tie rule; the
//                   window's f values live in a per-wave LDS ring
//   k_chain_fkeys   key = (group << 26) | (2^26 - 1 - f), value = sorted index;
//   sort            radix_sort_pairs32: the visiting order (f descending, index)
//   k_chain_walk    one lane per group walks and marks; each anchor is marked
//                   once, so the walk is O(A).  A chain's record is left at its
//                   head's visiting slot, every anchor gets that slot and its
//                   depth below the head
//   scan            exclusive_scan<uint32_t> of the kept flags: chain index
//   k_chain_compact records -> chain order, the groups' chain offsets
//   scan            exclusive_scan<uint32_t> of the chains' sizes: member offsets
//   k_chain_members anchor -> its place in its chain's member list
// No atomics decide an order: chains come out in visiting order by construction.
// (One atomic per group sums the DP's evaluated predecessors, a statistic.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "device.h"

namespace bwtmi {

namespace {

constexpr int kChainMaxPred = 4096;                    // max_pred's ceiling: the DP's ring of f values is 16 KiB at most
constexpr int kChainFBits = 26;                        // qe <= 2^24: f <= len + (qe - qe_first) <= 2^25
constexpr uint32_t kChainFMax = (1u << kChainFBits) - 1u;
constexpr uint32_t kChainNone = 0xffffffffu;

inline int chain_bits_for(int64_t values) {   // bits that hold 0 .. values - 1
    int b = 1;
    while (b < 63 && (int64_t{1} << b) < values) ++b;
    return b;
}

__global__ __launch_bounds__(256) void k_chain_keys(const int32_t *__restrict__ q, const int64_t *__restrict__ r,
                                                    const int32_t *__restrict__ len, int64_t na, int qbits,
                                                    uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= na) return;
    keys[t] = ((uint64_t)(r[t] + len[t]) << qbits) | (uint64_t)(q[t] + len[t]);
    vals[t] = (uint32_t)t;
}

__global__ __launch_bounds__(256) void k_chain_gkeys(const int64_t *__restrict__ group_off, int64_t ng,
                                                     const uint32_t *__restrict__ vals, int64_t na,
                                                     uint32_t *__restrict__ gk) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= na) return;
    gk[t] = (uint32_t)owner_of(ng, (int64_t)vals[t], [&](int64_t i) { return group_off[i]; });
}

__global__ __launch_bounds__(256) void k_chain_gather(const uint32_t *__restrict__ vals, const int32_t *__restrict__ q,
                                                      const int64_t *__restrict__ r, const int32_t *__restrict__ len,
                                                      int64_t na, int32_t *__restrict__ s_qe, int64_t *__restrict__ s_re,
                                                      int32_t *__restrict__ s_len) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= na) return;
    const uint32_t i = vals[t];
    const int32_t l = len[i];
    s_qe[t] = q[i] + l;
    s_re[t] = r[i] + l;
    s_len[t] = l;
}

__device__ __forceinline__ int32_t chain_cost(int32_t d) {   // d >= 0
    return d == 0 ? 0 : (d >> 4) + ((32 - __clz(d)) >> 1);
}

// the wave's maximum of a 64-bit key, as a scalar
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint64_t o = __shfl_xor((unsigned long long)v, m, 64);
        v = o > v ? o : v;
    }
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (uint64_t)hi << 32 | lo;
}

// One workgroup of one wave per group.  Every loop bound and exit is a scalar
// (Guard): the group's range and the anchor's own fields come from
// wave-uniform addresses, the window's winner from readfirstlane, the max_gap
// break from a ballot.  f and pred are indexed by sorted position; pred is
// relative to the group's first anchor.  The ring (dynamic LDS) holds ring_mask + 1
// >= max_pred values, a power of two: anchor i's slot is that of i - (ring_mask + 1),
// which no later anchor reads, and lane 0 writes it after the anchor's own reads.
__global__ __launch_bounds__(64) void k_chain_dp(const int64_t *__restrict__ group_off,
                                                 const int32_t *__restrict__ s_qe, const int64_t *__restrict__ s_re,
                                                 const int32_t *__restrict__ s_len, int32_t max_gap, int32_t bandwidth,
                                                 int32_t max_pred, int32_t ring_mask, int32_t *__restrict__ f,
                                                 int32_t *__restrict__ pred,
                                                 unsigned long long *__restrict__ evals) {
    extern __shared__ int32_t ring[];
    const int lane = (int)threadIdx.x;
    const int64_t a0 = group_off[blockIdx.x];
    const int32_t A = (int32_t)(group_off[blockIdx.x + 1] - a0);
    const int32_t *qe = s_qe + a0, *ln = s_len + a0;
    const int64_t *re = s_re + a0;
    uint32_t ev = 0;
    for (int32_t i = 0; i < A; ++i) {
        const int32_t qi = qe[i], li = ln[i];
        const int64_t ri = re[i];
        const int32_t lo = i > max_pred ? i - max_pred : 0;
        int32_t best = li, bp = -1;
        for (int32_t top = i - 1; top >= lo; top -= 64) {
            const int32_t j = top - lane;
            uint64_t key = 0;
            bool far = false;
            if (j >= lo) {
                const int64_t dr = ri - re[j];
                far = dr > (int64_t)max_gap;
                if (!far) {
                    ++ev;
                    const int32_t dq = qi - qe[j];
                    if (dq > 0 && dr > 0 && dq <= max_gap) {
                        const int32_t d = dq > (int32_t)dr ? dq - (int32_t)dr : (int32_t)dr - dq;
                        if (d <= bandwidth) {
                            const int32_t s = ring[j & ring_mask] + min(li, min(dq, (int32_t)dr)) - chain_cost(d);
                            if (s > li) key = (uint64_t)(uint32_t)s << 32 | (uint32_t)j;
                        }
                    }
                }
            }
            if (__ballot(key != 0) != 0) {
                const uint64_t w = wave_max_u64(key);
                // a later window holds farther predecessors: it wins only with a higher score
                if ((int32_t)(w >> 32) > best) {
                    best = (int32_t)(w >> 32);
                    bp = (int32_t)(uint32_t)w;
                }
            }
            if (__ballot(far) != 0) break;   // sorted by re: nothing further can qualify
        }
        if (lane == 0) {
            ring[i & ring_mask] = best;
            f[a0 + i] = best;
            pred[a0 + i] = bp;
        }
        __syncthreads();   // one wave: orders lane 0's ring store before the next anchor's loads
    }
    unsigned long long tot = ev;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) tot += __shfl_xor(tot, m, 64);
    if (lane == 0 && tot) atomicAdd(evals, tot);
}

__global__ __launch_bounds__(256) void k_chain_fkeys(const int64_t *__restrict__ group_off, int64_t ng,
                                                     const int32_t *__restrict__ f, int64_t na,
                                                     uint64_t *__restrict__ keys, uint32_t *__restrict__ vis) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= na) return;
    const uint64_t g = (uint64_t)owner_of(ng, t, [&](int64_t i) { return group_off[i]; });
    keys[t] = g << kChainFBits | (uint64_t)(kChainFMax - (uint32_t)f[t]);
    vis[t] = (uint32_t)t;
}

// per-slot record of a chain, left at its head's visiting slot
struct ChainCols {
    int32_t *score, *n, *qs, *qe;
    int64_t *rs, *re;
};

// One lane per group: the contract's extraction.  slot[] (all kChainNone on
// entry) is the used mark.  keep[] is all 0 on entry.
__global__ __launch_bounds__(64) void k_chain_walk(const int64_t *__restrict__ group_off, int64_t ng,
                                                   const uint32_t *__restrict__ vis, const int32_t *__restrict__ f,
                                                   const int32_t *__restrict__ pred, const int32_t *__restrict__ s_qe,
                                                   const int64_t *__restrict__ s_re, const int32_t *__restrict__ s_len,
                                                   int32_t min_score, int32_t min_anchors, uint32_t *__restrict__ slot,
                                                   uint32_t *__restrict__ depth, uint32_t *__restrict__ keep,
                                                   ChainCols rec) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ng) return;
    const int64_t a0 = group_off[g], a1 = group_off[g + 1];
    for (int64_t t = a0; t < a1; ++t) {
        const int64_t head = vis[t];
        if (slot[head] != kChainNone) continue;
        int64_t k = head;
        int32_t n = 0, below = 0, qs = INT32_MAX, qe = 0;
        int64_t rs = INT64_MAX, re = 0;
        for (;;) {
            slot[k] = (uint32_t)t;
            depth[k] = (uint32_t)n++;
            const int32_t l = s_len[k];
            qs = min(qs, s_qe[k] - l);
            qe = max(qe, s_qe[k]);
            rs = min(rs, s_re[k] - l);
            re = max(re, s_re[k]);
            const int32_t p = pred[k];
            if (p < 0) break;
            const int64_t u = a0 + p;
            if (slot[u] != kChainNone) {   // stop in front of a used anchor
                below = f[u];
                break;
            }
            k = u;
        }
        const int32_t score = f[head] - below;
        rec.score[t] = score;
        rec.n[t] = n;
        rec.qs[t] = qs;
        rec.qe[t] = qe;
        rec.rs[t] = rs;
        rec.re[t] = re;
        if (score >= min_score && n >= min_anchors) keep[t] = 1u;
    }
}

// thread t < na: a kept chain's record to row cidx[t]; thread t <= ng: group t's first chain
__global__ __launch_bounds__(256) void k_chain_compact(const int64_t *__restrict__ group_off, int64_t ng, int64_t na,
                                                       const uint32_t *__restrict__ keep,
                                                       const uint32_t *__restrict__ cidx, ChainCols rec, ChainCols out,
                                                       uint32_t *__restrict__ nmem, int64_t *__restrict__ chain_off) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t <= ng) chain_off[t] = (int64_t)cidx[group_off[t]];
    if (t >= na || !keep[t]) return;
    const uint32_t c = cidx[t];
    out.score[c] = rec.score[t];
    out.n[c] = rec.n[t];
    out.qs[c] = rec.qs[t];
    out.qe[c] = rec.qe[t];
    out.rs[c] = rec.rs[t];
    out.re[c] = rec.re[t];
    nmem[c] = (uint32_t)rec.n[t];
}

// thread a < na (sorted position): an anchor of a kept chain goes to its place,
// counted from the chain's end by its depth below the head
__global__ __launch_bounds__(256) void k_chain_members(int64_t na, const uint32_t *__restrict__ slot,
                                                       const uint32_t *__restrict__ depth,
                                                       const uint32_t *__restrict__ keep,
                                                       const uint32_t *__restrict__ cidx,
                                                       const uint32_t *__restrict__ moff,
                                                       const uint32_t *__restrict__ order, int64_t *__restrict__ member) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= na) return;
    const uint32_t t = slot[a];
    if (t == kChainNone || !keep[t]) return;
    const uint32_t c = cidx[t];
    member[(int64_t)moff[c + 1] - 1 - (int64_t)depth[a]] = (int64_t)order[a];
}

// carves one slot into arrays (256-byte aligned)
struct Arena {
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

void chain_anchors_device(Ctx &c, const int64_t *group_off, int64_t ng, const int32_t *q, const int64_t *r,
                          const int32_t *len, const ChainParams &p, ChainResult &out) {
    out.chain_off.assign((size_t)ng + 1, 0);
    out.score.clear();
    out.n_anchors.clear();
    out.qstart.clear();
    out.qend.clear();
    out.rstart.clear();
    out.rend.clear();
    out.member_off.assign(1, 0);
    out.member.clear();
    out.evals = 0;
    const int64_t na = ng > 0 ? group_off[ng] : 0;
    if (na == 0) return;
    if (na >= (int64_t{1} << 31) || ng >= (int64_t{1} << 31))
        fail(BWTMI_E_NOMEM, "chain: %lld anchors in %lld groups exceed the 2^31 the chainer indexes", (long long)na,
             (long long)ng);
    int64_t max_qe = 0, max_re = 0;
    for (int64_t i = 0; i < na; ++i) {
        max_qe = std::max<int64_t>(max_qe, (int64_t)q[i] + len[i]);
        max_re = std::max<int64_t>(max_re, r[i] + len[i]);
    }
    const int qbits = chain_bits_for(max_qe + 1), rbits = chain_bits_for(max_re + 1), gbits = chain_bits_for(ng);

    // ---- one slot, carved.  The chain rows reuse the uploaded anchors' space
    // (free after k_chain_gather) and the first sort's group keys.
    Arena ar;
    const size_t N = (size_t)na;
    const size_t o_goff = ar.take((size_t)(ng + 1) * 8), o_q = ar.take(N * 4), o_r = ar.take(N * 8), o_len = ar.take(N * 4);
    const size_t o_keys = ar.take(N * 8), o_order = ar.take(N * 4), o_gk = ar.take(N * 4);
    const size_t o_sqe = ar.take(N * 4), o_sre = ar.take(N * 8), o_slen = ar.take(N * 4);
    const size_t o_f = ar.take(N * 4), o_pred = ar.take(N * 4), o_vis = ar.take(N * 4);
    const size_t o_slot = ar.take(N * 4), o_depth = ar.take(N * 4), o_keep = ar.take((N + 1) * 4), o_cidx = ar.take((N + 1) * 4);
    const size_t o_ts = ar.take(N * 4), o_tn = ar.take(N * 4), o_tqs = ar.take(N * 4), o_tqe = ar.take(N * 4);
    const size_t o_trs = ar.take(N * 8), o_tre = ar.take(N * 8);
    const size_t o_cqe = ar.take(N * 4), o_cre = ar.take(N * 8);
    const size_t o_nmem = ar.take((N + 1) * 4), o_moff = ar.take((N + 1) * 4), o_member = ar.take(N * 8);
    const size_t o_coff = ar.take((size_t)(ng + 1) * 8), o_ev = ar.take(8);
    c.slot[S_IDX0].ensure(ar.used);
    ar.base = c.slot[S_IDX0].as<uint8_t>();
    int64_t *d_goff = ar.at<int64_t>(o_goff), *d_r = ar.at<int64_t>(o_r);
    int32_t *d_q = ar.at<int32_t>(o_q), *d_len = ar.at<int32_t>(o_len);
    uint64_t *d_keys = ar.at<uint64_t>(o_keys);
    uint32_t *d_order = ar.at<uint32_t>(o_order), *d_gk = ar.at<uint32_t>(o_gk), *d_vis = ar.at<uint32_t>(o_vis);
    int32_t *d_sqe = ar.at<int32_t>(o_sqe), *d_slen = ar.at<int32_t>(o_slen), *d_f = ar.at<int32_t>(o_f);
    int32_t *d_pred = ar.at<int32_t>(o_pred);
    int64_t *d_sre = ar.at<int64_t>(o_sre);
    uint32_t *d_slot = ar.at<uint32_t>(o_slot), *d_depth = ar.at<uint32_t>(o_depth), *d_keep = ar.at<uint32_t>(o_keep);
    uint32_t *d_cidx = ar.at<uint32_t>(o_cidx), *d_nmem = ar.at<uint32_t>(o_nmem), *d_moff = ar.at<uint32_t>(o_moff);
    const ChainCols rec{ar.at<int32_t>(o_ts), ar.at<int32_t>(o_tn), ar.at<int32_t>(o_tqs), ar.at<int32_t>(o_tqe),
                        ar.at<int64_t>(o_trs), ar.at<int64_t>(o_tre)};
    const ChainCols row{d_q, d_len, (int32_t *)d_gk, ar.at<int32_t>(o_cqe), d_r, ar.at<int64_t>(o_cre)};
    int64_t *d_member = ar.at<int64_t>(o_member), *d_coff = ar.at<int64_t>(o_coff);
    auto *d_ev = ar.at<unsigned long long>(o_ev);

    hipStream_t st = c.stream;
    // timed like a kernel (statistics name chain_upload): what the mapper's re-upload of its seeds costs
    c.kbegin("chain_upload", (double)na * 16.0 + (double)(ng + 1) * 8.0);
    HIPCHECK(hipMemcpyAsync(d_goff, group_off, (size_t)(ng + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_q, q, N * 4, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_r, r, N * 8, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_len, len, N * 4, hipMemcpyHostToDevice, st));
    c.kend();
    HIPCHECK(hipMemsetAsync(d_slot, 0xff, N * 4, st));
    HIPCHECK(hipMemsetAsync(d_keep, 0, (N + 1) * 4, st));
    HIPCHECK(hipMemsetAsync(d_ev, 0, 8, st));

    // ---- the contract's order: (group, re, qe), ties in input order
    KLAUNCH("k_chain_keys", (double)na * 28.0, k_chain_keys, dim3(blocks(na)), dim3(256), 0, st, d_q, d_r, d_len, na,
            qbits, d_keys, d_order);
    HIPCHECK(hipGetLastError());
    radix_sort_pairs32(c, d_keys, d_order, na, 0, qbits + rbits);
    if (ng > 1) {
        KLAUNCH("k_chain_gkeys", (double)na * 8.0, k_chain_gkeys, dim3(blocks(na)), dim3(256), 0, st, d_goff, ng, d_order,
                na, d_gk);
        HIPCHECK(hipGetLastError());
        radix_sort_pairs_k32(c, d_gk, d_order, na, 0, gbits);
    }
    KLAUNCH("k_chain_gather", (double)na * 36.0, k_chain_gather, dim3(blocks(na)), dim3(256), 0, st, d_order, d_q, d_r,
            d_len, na, d_sqe, d_sre, d_slen);
    HIPCHECK(hipGetLastError());

    // ---- the DP (bytes: the anchor's own 16, 8 out; the window is re-read from cache)
    if (p.max_pred < 1 || p.max_pred > kChainMaxPred) fail(BWTMI_E_ARG, "chain: max_pred %d outside 1..4096", (int)p.max_pred);
    int ring = 64;
    while (ring < p.max_pred) ring *= 2;
    KLAUNCH("k_chain_dp", (double)na * 24.0, k_chain_dp, dim3((unsigned)ng), dim3(64), (size_t)ring * 4, st, d_goff, d_sqe,
            d_sre, d_slen, p.max_gap, p.bandwidth, p.max_pred, ring - 1, d_f, d_pred, d_ev);
    HIPCHECK(hipGetLastError());

    // ---- extraction
    KLAUNCH("k_chain_fkeys", (double)na * 16.0, k_chain_fkeys, dim3(blocks(na)), dim3(256), 0, st, d_goff, ng, d_f, na,
            d_keys, d_vis);
    HIPCHECK(hipGetLastError());
    radix_sort_pairs32(c, d_keys, d_vis, na, 0, kChainFBits + gbits);
    KLAUNCH("k_chain_walk", (double)na * 60.0, k_chain_walk, dim3(blocks(ng, 64)), dim3(64), 0, st, d_goff, ng, d_vis, d_f,
            d_pred, d_sqe, d_sre, d_slen, p.min_score, p.min_anchors, d_slot, d_depth, d_keep, rec);
    HIPCHECK(hipGetLastError());
    exclusive_scan<uint32_t>(c, d_keep, d_cidx, na + 1);
    uint32_t *mb = c.mailbox<uint32_t>(2);
    unsigned long long *mb_ev = reinterpret_cast<unsigned long long *>(mb + 2);
    HIPCHECK(hipMemcpyAsync(mb, d_cidx + na, 4, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(mb_ev, d_ev, 8, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemsetAsync(d_nmem, 0, (N + 1) * 4, st));
    KLAUNCH("k_chain_compact", (double)na * 8.0, k_chain_compact, dim3(blocks(std::max(na, ng + 1))), dim3(256), 0, st,
            d_goff, ng, na, d_keep, d_cidx, rec, row, d_nmem, d_coff);
    HIPCHECK(hipGetLastError());
    scan_wait(st);   // (the uploads above read the caller's pageable arrays: they are done too)
    const int64_t nchain = mb[0];
    out.evals = (int64_t)*mb_ev;
    if (nchain > na) fail(BWTMI_E_STATE, "chain: %lld chains out of %lld anchors", (long long)nchain, (long long)na);
    HIPCHECK(hipMemcpyAsync(out.chain_off.data(), d_coff, (size_t)(ng + 1) * 8, hipMemcpyDeviceToHost, st));
    std::vector<uint32_t> moff;
    if (nchain > 0) {
        exclusive_scan<uint32_t>(c, d_nmem, d_moff, nchain + 1);
        KLAUNCH("k_chain_members", (double)na * 28.0, k_chain_members, dim3(blocks(na)), dim3(256), 0, st, na, d_slot,
                d_depth, d_keep, d_cidx, d_moff, d_order, d_member);
        HIPCHECK(hipGetLastError());
        const size_t C = (size_t)nchain;
        out.score.resize(C);
        out.n_anchors.resize(C);
        out.qstart.resize(C);
        out.qend.resize(C);
        out.rstart.resize(C);
        out.rend.resize(C);
        moff.resize(C + 1);
        HIPCHECK(hipMemcpyAsync(out.score.data(), row.score, C * 4, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipMemcpyAsync(out.n_anchors.data(), row.n, C * 4, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipMemcpyAsync(out.qstart.data(), row.qs, C * 4, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipMemcpyAsync(out.qend.data(), row.qe, C * 4, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipMemcpyAsync(out.rstart.data(), row.rs, C * 8, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipMemcpyAsync(out.rend.data(), row.re, C * 8, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipMemcpyAsync(moff.data(), d_moff, (C + 1) * 4, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));
        const int64_t nmember = moff[C];
        if (nmember > na) fail(BWTMI_E_STATE, "chain: %lld members out of %lld anchors", (long long)nmember, (long long)na);
        out.member_off.assign(moff.begin(), moff.end());
        out.member.resize((size_t)nmember);
        HIPCHECK(hipMemcpyAsync(out.member.data(), d_member, (size_t)nmember * 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHECK(hipStreamSynchronize(st));
}

void index_map_batch(Ctx &c, DeviceIndex *ix, const uint8_t *qs, const int64_t *off, int64_t nq, int32_t min_len,
                     bool both_strands, bool long_entry, int64_t max_occ, int64_t max_positions, const ChainParams &p,
                     MapResult &out) {
    out = MapResult{};
    out.chain_off.assign((size_t)std::max<int64_t>(nq, 0) + 1, 0);
    out.member_off.assign(1, 0);
    SmemResult sm;
    try {
        if (long_entry) index_smem_long_batch(c, ix, qs, off, nq, min_len, both_strands, max_occ, max_positions, sm);
        else index_smem_batch(c, ix, qs, off, nq, min_len, both_strands, max_occ, max_positions, sm);
    } catch (...) {
        out.positions_total = sm.positions_total;
        throw;
    }
    out.positions_total = sm.positions_total;
    const int64_t nsmem = (int64_t)sm.qstart.size();
    if (sm.pos_off.size() != (size_t)nsmem + 1) sm.pos_off.assign((size_t)nsmem + 1, 0);   // (no SMEMs: [0])

    // ---- anchors: one per listed position, in the searched string's coordinates;
    // group = 2 * query + strand.  The SMEMs come by (query, strand), so the
    // anchors are already grouped.
    const int64_t na = (int64_t)sm.pos.size(), ng = 2 * nq;
    std::vector<int64_t> goff((size_t)ng + 1, 0), ar((size_t)na);
    std::vector<int32_t> aq((size_t)na), al((size_t)na);
    for (int64_t qi = 0; qi < nq; ++qi) {
        const int32_t m = (int32_t)(off[qi + 1] - off[qi]);
        for (int64_t s = sm.smem_off[(size_t)qi]; s < sm.smem_off[(size_t)qi + 1]; ++s) {
            const int64_t a = sm.pos_off[(size_t)s], b = sm.pos_off[(size_t)s + 1];
            if (a == b) {   // above max_occ (a listed SMEM occurs at least once)
                ++out.skipped_smems;
                continue;
            }
            const int32_t l = sm.qend[(size_t)s] - sm.qstart[(size_t)s];
            const int32_t sq = sm.strand[(size_t)s] ? m - sm.qend[(size_t)s] : sm.qstart[(size_t)s];
            goff[(size_t)(2 * qi + sm.strand[(size_t)s]) + 1] += b - a;
            for (int64_t k = a; k < b; ++k) {
                aq[(size_t)k] = sq;
                ar[(size_t)k] = sm.pos[(size_t)k];
                al[(size_t)k] = l;
            }
        }
    }
    for (int64_t g = 0; g < ng; ++g) goff[(size_t)g + 1] += goff[(size_t)g];
    out.anchors = na;

    ChainResult ch;
    chain_anchors_device(c, goff.data(), ng, aq.data(), ar.data(), al.data(), p, ch);
    out.evals = ch.evals;

    // ---- back to the original queries' coordinates
    const int64_t nchain = (int64_t)ch.score.size();
    for (int64_t qi = 0; qi <= nq; ++qi) out.chain_off[(size_t)qi] = ch.chain_off[(size_t)(2 * qi)];
    out.strand.resize((size_t)nchain);
    out.score = std::move(ch.score);
    out.n_anchors = std::move(ch.n_anchors);
    out.qstart.resize((size_t)nchain);
    out.qend.resize((size_t)nchain);
    out.rstart = std::move(ch.rstart);
    out.rend = std::move(ch.rend);
    out.member_off = std::move(ch.member_off);
    const size_t nm = ch.member.size();
    out.mq.resize(nm);
    out.mr.resize(nm);
    out.mlen.resize(nm);
    for (int64_t g = 0; g < ng; ++g) {
        const int32_t m = (int32_t)(off[g / 2 + 1] - off[g / 2]);
        const bool rev = (g & 1) != 0;
        for (int64_t k = ch.chain_off[(size_t)g]; k < ch.chain_off[(size_t)g + 1]; ++k) {
            out.strand[(size_t)k] = rev ? 1 : 0;
            out.qstart[(size_t)k] = rev ? m - ch.qend[(size_t)k] : ch.qstart[(size_t)k];
            out.qend[(size_t)k] = rev ? m - ch.qstart[(size_t)k] : ch.qend[(size_t)k];
            for (int64_t t = out.member_off[(size_t)k]; t < out.member_off[(size_t)k + 1]; ++t) {
                const int64_t a = ch.member[(size_t)t];
                out.mq[(size_t)t] = rev ? m - aq[(size_t)a] - al[(size_t)a] : aq[(size_t)a];
                out.mr[(size_t)t] = ar[(size_t)a];
                out.mlen[(size_t)t] = al[(size_t)a];
            }
        }
    }
}

}  // namespace bwtmi
