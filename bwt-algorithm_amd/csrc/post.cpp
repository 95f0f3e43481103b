// post.cpp -- exact host restatement of the repeat post-processing
// (TandemRepeatFinder, bwt.py:3144-3944) over the raw strict hits.
//
// Work is organised per "fold unit": the contigs whose natural sort keys are
// equal (normally exactly one contig).  Every stage of the reference either
// groups by chromosome or folds over the globally sorted list with a
// same-chromosome test, so units are independent.  Inside a unit every stage
// is either data-parallel (nested-suppression queries) or part of the one
// sequential fold-to-filter pass (fold_cuts), which runs in parallel over the
// segments between verified cuts: each segment gets the exact sequential
// result, so the output does not depend on thread count.
//
// Records travel as compact Items: a strict hit (bwt.py:1952-1993) is fully
// determined by (start, end, motif length, copies) -- its motif is a slice of
// the contig, confidence 0.95, mismatch 0, ... -- so only records produced by
// _recompute_repeat carry an Extra with their own fields.  actual_sequence is
// always the current frame's slice [start, end) (trimmed before
// _restore_reference_coordinates, full after), so it is never stored.
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <functional>
#include <memory>
#include <string>
#include <string_view>
#include <thread>
#include <type_traits>
#include <vector>

#include <sched.h>

#include "common.h"

namespace bwtmi {

// CPUs this process may use: the affinity mask, capped by a cgroup CPU quota
static int cpus_visible() {
    int n = 0;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
    if (n <= 0) n = (int)std::max(1u, std::thread::hardware_concurrency());
    long q = -1, per = -1;
    if (FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {   // cgroup v2: "max 100000" or "Q P"
        char a[32] = {0};
        long b = 0;
        if (std::fscanf(f, "%31s %ld", a, &b) == 2 && std::strcmp(a, "max") != 0) {
            q = std::atol(a);
            per = b;
        }
        std::fclose(f);
    } else if (FILE *g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {   // cgroup v1
        if (std::fscanf(g, "%ld", &q) != 1) q = -1;
        std::fclose(g);
        if (FILE *h = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
            if (std::fscanf(h, "%ld", &per) != 1) per = -1;
            std::fclose(h);
        }
    }
    if (q > 0 && per > 0) n = std::min<int>(n, (int)std::max<long>(1, (q + per - 1) / per));
    return n;
}

int host_cpu_budget(int *visible, int *local_world) {
    static const int vis = cpus_visible();
    static const int lw = [] {
        const char *e = std::getenv("LOCAL_WORLD_SIZE");
        const int v = e ? std::atoi(e) : 1;
        return v > 0 ? v : 1;
    }();
    if (visible) *visible = vis;
    if (local_world) *local_world = lw;
    return std::max(1, std::min(16, vis / lw));   // 16 measured fastest per rank
}

int host_threads(const bwtmi_params &p) {
    if (p.threads > 0) return p.threads;
    return host_cpu_budget(nullptr, nullptr);
}

// ------------------------------------------------------------ NUMA placement
// The CPU set host work runs on (empty: unchanged).  Set once per process by
// bind_host_numa; the calling thread takes it at once, pool workers at the
// start of their next region (they may predate the binding).
namespace {
std::mutex g_bind_mu;
cpu_set_t g_bind_set;
std::atomic<int> g_bind_epoch{0};
thread_local int tl_bind_epoch = 0;
inline void apply_binding() {
    const int e = g_bind_epoch.load(std::memory_order_acquire);
    if (e == tl_bind_epoch) return;
    cpu_set_t cs;
    {
        std::lock_guard<std::mutex> lk(g_bind_mu);
        cs = g_bind_set;
    }
    (void)sched_setaffinity(0, sizeof cs, &cs);
    tl_bind_epoch = e;
}
}  // namespace

std::string cpulist_str(const cpu_set_t &cs) {
    std::string s;
    for (int c = 0; c < CPU_SETSIZE; ++c) {
        if (!CPU_ISSET(c, &cs)) continue;
        int e = c;
        while (e + 1 < CPU_SETSIZE && CPU_ISSET(e + 1, &cs)) ++e;
        if (!s.empty()) s += ',';
        s += std::to_string(c);
        if (e > c) s += '-' + std::to_string(e);
        c = e;
    }
    return s;
}
bool parse_cpulist(const char *txt, cpu_set_t &cs) {
    CPU_ZERO(&cs);
    for (const char *p = txt; p && *p && *p != '\n';) {
        char *e;
        const long a = std::strtol(p, &e, 10);
        if (e == p) return false;
        long b = a;
        p = e;
        if (*p == '-') {
            b = std::strtol(p + 1, &e, 10);
            if (e == p + 1) return false;
            p = e;
        }
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c) CPU_SET((int)c, &cs);
        if (*p == ',') ++p;
    }
    return true;
}
namespace {
int read_int(const std::string &path, int def) {
    int v = def;
    if (FILE *f = std::fopen(path.c_str(), "r")) {
        if (std::fscanf(f, "%d", &v) != 1) v = def;
        std::fclose(f);
    }
    return v;
}
int g_bound_node = -1;   // the node host work is bound to (under g_bind_mu)
cpu_set_t g_orig_set;    // the affinity the first binding replaced
}  // namespace

// The NUMA node of a GPU from its PCI address ("0000:75:00.0"), -1 unknown
int gpu_numa_node(const char *sysroot, const char *pci) {
    std::string id(pci ? pci : "");
    for (auto &ch : id) ch = (char)std::tolower((unsigned char)ch);
    return read_int(std::string(sysroot) + "/bus/pci/devices/" + id + "/numa_node", -1);
}

// Pure planner (no affinity change; sysfs read under `sysroot`, "/sys" on a
// host, a faked tree in the tests).  Local rank r of the node drives the GPU
// at rank_pci[r]; this rank's GPU is rank_pci[local_rank].  The set: the
// `allowed` CPUs of this GPU's NUMA node; with one hardware thread per
// physical core when those cores can hold every local rank WHOSE GPU SITS ON
// THAT NODE with `threads` workers + 4 runtime threads each (two workers on
// the siblings of one core run the memory-bound host passes at well under
// half speed each; smt keeps the siblings).  False (no binding): unknown
// node, the process already runs inside the node, or fewer allowed CPUs there
// than `threads` (a small cpuset split over both nodes).
bool plan_host_binding(const char *sysroot, int local_rank, const std::vector<std::string> &rank_pci, int threads,
                       bool smt, const cpu_set_t &allowed, cpu_set_t &out, int *node_out, int *ranks_on_node) {
    if (local_rank < 0 || local_rank >= (int)rank_pci.size()) return false;
    const int node = gpu_numa_node(sysroot, rank_pci[(size_t)local_rank].c_str());
    if (node_out) *node_out = node;
    if (node < 0) return false;
    int peers = 0;
    for (const auto &p : rank_pci) peers += gpu_numa_node(sysroot, p.c_str()) == node;
    if (ranks_on_node) *ranks_on_node = peers;
    cpu_set_t want, both;
    FILE *f = std::fopen((std::string(sysroot) + "/devices/system/node/node" + std::to_string(node) + "/cpulist").c_str(), "r");
    if (!f) return false;
    char buf[4096];
    const bool ok = std::fgets(buf, sizeof buf, f) != nullptr;
    std::fclose(f);
    if (!ok || !parse_cpulist(buf, want)) return false;
    CPU_AND(&both, &want, &allowed);
    if (CPU_EQUAL(&both, &allowed) || CPU_COUNT(&both) < threads) return false;
    if (!smt) {
        cpu_set_t one;
        CPU_ZERO(&one);
        std::vector<std::pair<int, int>> seen;   // (package, core) taken
        for (int c = 0; c < CPU_SETSIZE; ++c) {
            if (!CPU_ISSET(c, &both)) continue;
            const std::string t = std::string(sysroot) + "/devices/system/cpu/cpu" + std::to_string(c) + "/topology/";
            const int pkg = read_int(t + "physical_package_id", -1), core = read_int(t + "core_id", -1);
            if (pkg < 0 || core < 0) { CPU_ZERO(&one); break; }   // no topology: keep the node set
            if (std::find(seen.begin(), seen.end(), std::make_pair(pkg, core)) != seen.end()) continue;
            seen.emplace_back(pkg, core);
            CPU_SET(c, &one);
        }
        if (CPU_COUNT(&one) >= peers * (threads + 4)) both = one;
    }
    out = both;
    return true;
}

bool bind_host_numa(int local_rank, const std::vector<std::string> &rank_pci) {
    cpu_set_t cur, want;
    if (sched_getaffinity(0, sizeof cur, &cur) != 0) return false;
    int node = -1;
    if (!plan_host_binding("/sys", local_rank, rank_pci, host_cpu_budget(nullptr, nullptr), knob(KN_NUMA_SMT) != 0, cur,
                           want, &node, nullptr))
        return false;
    {
        std::lock_guard<std::mutex> lk(g_bind_mu);
        if (g_bound_node >= 0 && g_bound_node != node) return false;   // contexts on two nodes: keep the first
        if (g_bound_node < 0) g_orig_set = cur;
        g_bound_node = node;
        g_bind_set = want;
    }
    g_bind_epoch.fetch_add(1, std::memory_order_acq_rel);
    apply_binding();
    return true;
}

bool unbind_host() {
    {
        std::lock_guard<std::mutex> lk(g_bind_mu);
        if (g_bound_node < 0) return false;
        g_bound_node = -1;
        g_bind_set = g_orig_set;
    }
    g_bind_epoch.fetch_add(1, std::memory_order_acq_rel);
    apply_binding();
    return true;
}

// Persistent worker pools: parallel regions reuse the same threads (and their
// thread-local DP scratch) instead of spawning per call.  The caller takes
// part as worker 0; a region started from inside a worker of the same pool
// runs inline.  Parallel regions go to the calling thread's current pool (the
// process-wide one unless the thread belongs to a unit group, postprocess).
namespace {
// Region hand-off: a region is published by bumping `agen`; workers that
// finished their last region may spin on it for a while (BWTMI_POOL_SPIN_US)
// before they block on the condition variable, and the caller spins on
// `apending` the same way before it blocks.  10 us catches the back-to-back
// regions of a step (r03aa/r03ab: C3 +4 %, W=8 shard step 8.0-8.1 vs 8.6-8.9
// ms), while a 60 us spin, also held through longer serial parts, cost the C3
// line ~7 % on another box (r03z).  Auto (-1, the default): 200 us while the
// calling job holds <= 32 Mbp (its regions are short and come back to back:
// W=8 shard 6.3-6.6 vs 6.8-7.3 ms at 10 us, r05gd), else 10 us (C3 within
// its run-to-run spread either way; round 6 tried 300 us: r06y favoured it,
// but interleaved after a warm-up run on one box, r06ar, 300 us 3582 / 3543 /
// 3679 vs 10 us 3447 / 3615 / 3767 Mbp/s -- no gain, more CPU).  0 = block at once.
std::atomic<int64_t> g_auto_spin_ns{10000};
inline int64_t pool_spin_ns() {
    const int64_t k = knob(KN_POOL_SPIN_US);
    return k >= 0 ? k * 1000 : g_auto_spin_ns.load(std::memory_order_relaxed);
}
inline int64_t now_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// spin until pred() or the spin window ends; true when pred() held
template <class P>
inline bool spin_until(P &&pred) {
    const int64_t lim = pool_spin_ns();
    if (lim <= 0) return pred();
    const int64_t t0 = now_ns();
    for (int k = 0;; ++k) {
        if (pred()) return true;
        __builtin_ia32_pause();
        if ((k & 63) == 63 && now_ns() - t0 > lim) return pred();
    }
}

class Pool {
public:
    static Pool &global() {
        static Pool p;
        return p;
    }
    static Pool &current() { return tl_pool ? *tl_pool : global(); }
    // f(w) for w in [0, nt)
    void run(int nt, const std::function<void(int)> &f) {
        if (nt <= 1 || worker_of == this) {
            for (int w = 0; w < nt; ++w) f(w);
            return;
        }
        std::unique_lock<std::mutex> region(region_mu);   // one region at a time
        grow(nt - 1);
        bool wake;
        {
            std::lock_guard<std::mutex> lk(mu);
            job = &f;
            want = nt - 1;
            err = nullptr;
            apending.store(nt - 1, std::memory_order_relaxed);
            agen.store(agen.load(std::memory_order_relaxed) + 1, std::memory_order_release);
            wake = sleepers > 0;
        }
        if (wake) cv.notify_all();
        Pool *const outer = worker_of;
        worker_of = this;
        try {
            f(0);
        } catch (...) {
            std::lock_guard<std::mutex> lk(mu);
            if (!err) err = std::current_exception();
        }
        worker_of = outer;
        // every worker finishes before f (and what it references) goes out of scope
        if (!spin_until([&] { return apending.load(std::memory_order_acquire) == 0; })) {
            std::unique_lock<std::mutex> lk(mu);
            caller_waits = true;
            done.wait(lk, [&] { return apending.load(std::memory_order_acquire) == 0; });
            caller_waits = false;
        }
        std::lock_guard<std::mutex> lk(mu);
        job = nullptr;
        if (err) {
            std::exception_ptr e = err;
            err = nullptr;
            std::rethrow_exception(e);
        }
    }
    ~Pool() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
            agen.store(agen.load(std::memory_order_relaxed) + 1, std::memory_order_release);
        }
        cv.notify_all();
        for (auto &t : th) t.join();
    }
    static thread_local Pool *tl_pool;   // the pool this thread's regions go to (nullptr: global)

private:
    void grow(int n) {
        while ((int)th.size() < n) {
            const int id = (int)th.size();
            th.emplace_back([this, id] { loop(id); });
        }
    }
    void loop(int id) {
        worker_of = this;
        tl_pool = this;
        int64_t seen = 0;
        {
            std::lock_guard<std::mutex> lk(mu);
            seen = agen.load(std::memory_order_relaxed);   // a worker created for the current region still takes part in it
            if (job && id < want) seen -= 1;
        }
        for (;;) {
            const std::function<void(int)> *f;
            if (!spin_until([&] { return agen.load(std::memory_order_acquire) != seen; })) {
                std::unique_lock<std::mutex> lk(mu);
                ++sleepers;
                cv.wait(lk, [&] { return agen.load(std::memory_order_relaxed) != seen; });
                --sleepers;
            }
            {
                std::lock_guard<std::mutex> lk(mu);   // job / want / stop of the generation seen
                if (stop) return;
                seen = agen.load(std::memory_order_relaxed);
                if (id >= want) continue;
                f = job;
            }
            apply_binding();
            try {
                (*f)(id + 1);
            } catch (...) {   // reported to the caller of run(); never escapes the thread
                std::lock_guard<std::mutex> lk(mu);
                if (!err) err = std::current_exception();
            }
            if (apending.fetch_sub(1, std::memory_order_acq_rel) == 1) {
                std::lock_guard<std::mutex> lk(mu);   // after the decrement: no lost wake-up
                if (caller_waits) done.notify_one();
            }
        }
    }
    std::vector<std::thread> th;
    std::mutex mu, region_mu;
    std::condition_variable cv, done;
    const std::function<void(int)> *job = nullptr;
    std::exception_ptr err;
    int want = 0, sleepers = 0;
    bool caller_waits = false;
    std::atomic<int64_t> agen{0};
    std::atomic<int> apending{0};
    bool stop = false;
    static thread_local Pool *worker_of;   // the pool whose region this thread is running
};
thread_local Pool *Pool::worker_of = nullptr;
thread_local Pool *Pool::tl_pool = nullptr;
}  // namespace

void pool_spin_for_job(const Job &job) {
    int64_t bases = 0;
    for (size_t i = 0; i < job.contigs.size(); ++i)
        if (job.selected.empty() || (i < job.selected.size() && job.selected[i])) bases += job.contigs[i].trimmed_len();
    g_auto_spin_ns.store(bases <= 32000000 ? 200000 : 10000, std::memory_order_relaxed);
}

// fn(begin, end) over [0, n) in contiguous chunks
template <class F>
static void parallel_for(int64_t n, int nt, F &&fn) {
    if (n <= 0) return;
    nt = (int)std::max<int64_t>(1, std::min<int64_t>(nt, (n + 1023) / 1024));
    if (nt <= 1) {
        fn((int64_t)0, n);
        return;
    }
    Pool::current().run(nt, [&](int t) { fn(n * t / nt, n * (t + 1) / nt); });
}

// dynamic scheduling: fn(item, worker)
template <class F>
static void parallel_items(int64_t n, int nt, F &&fn) {
    if (n <= 0) return;
    nt = (int)std::max<int64_t>(1, std::min<int64_t>(nt, n));
    std::atomic<int64_t> next{0};
    auto work = [&](int w) {
        for (;;) {
            const int64_t k = next.fetch_add(1, std::memory_order_relaxed);
            if (k >= n) break;
            fn(k, w);
        }
    };
    if (nt == 1) { work(0); return; }
    Pool::current().run(nt, work);
}

void run_tasks(int64_t n, int nt, const std::function<void(int64_t)> &fn) {
    parallel_items(n, nt, [&](int64_t k, int) { fn(k); });
}

// ------------------------------------------------------------ natural key
std::vector<NatPart> natural_key(const std::string &s) {      // bwt.py:22-36
    std::vector<NatPart> out;
    size_t i = 0, n = s.size();
    while (i < n) {
        size_t j = i;
        const bool dig = s[i] >= '0' && s[i] <= '9';
        while (j < n && ((s[j] >= '0' && s[j] <= '9') == dig)) ++j;
        NatPart p;
        p.digit = dig;
        if (dig) {
            size_t k = i;
            while (k + 1 < j && s[k] == '0') ++k;  // int(part): strip leading zeros
            p.text = s.substr(k, j - k);
        } else {
            p.text = s.substr(i, j - i);
            for (auto &c : p.text)
                if (c >= 'A' && c <= 'Z') c = (char)(c + 32);
        }
        out.push_back(std::move(p));
        i = j;
    }
    return out;
}

int natural_cmp(const std::vector<NatPart> &a, const std::vector<NatPart> &b) {
    const size_t n = std::min(a.size(), b.size());
    for (size_t i = 0; i < n; ++i) {
        const NatPart &x = a[i], &y = b[i];
        if (x.digit != y.digit) return x.digit ? -1 : 1;  // (0, int) < (1, str)
        if (x.digit && x.text.size() != y.text.size()) return x.text.size() < y.text.size() ? -1 : 1;
        const int c = x.text.compare(y.text);
        if (c) return c < 0 ? -1 : 1;
    }
    if (a.size() != b.size()) return a.size() < b.size() ? -1 : 1;
    return 0;
}

void Job::assign_units() {
    natkeys.clear();
    for (auto &c : contigs) natkeys.push_back(natural_key(c.name));
    std::vector<int32_t> order(contigs.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int32_t)i;
    std::stable_sort(order.begin(), order.end(),
                     [&](int32_t a, int32_t b) { return natural_cmp(natkeys[a], natkeys[b]) < 0; });
    nunits = 0;
    unit_rank.clear();
    for (size_t k = 0; k < order.size(); ++k) {
        if (k == 0 || natural_cmp(natkeys[order[k - 1]], natkeys[order[k]]) != 0) {
            unit_rank.push_back(nunits);
            ++nunits;
        }
        contigs[order[k]].unit = nunits - 1;   // unit ids are ranks by natural key
    }
}

std::vector<int32_t> shard_units(Job &job, int32_t world, int32_t rank) {
    job.assign_units();
    std::vector<int64_t> w((size_t)job.nunits, 0);
    for (auto &c : job.contigs) w[(size_t)c.unit] += c.weight;
    const std::vector<size_t> owner = lpt_assign(w, (size_t)std::max(1, world));
    std::vector<int32_t> out;
    for (size_t c = 0; c < job.contigs.size(); ++c)
        if (owner[(size_t)job.contigs[c].unit] == (size_t)rank) out.push_back((int32_t)c);
    return out;
}

namespace {

// fields of a record produced by _recompute_repeat (bwt.py:3593-3614)
struct Extra {                  // trivially destructible: strings live in the Pools arena
    std::string_view motif;     // == consensus_motif
    std::string_view variations;  // ';'-joined, empty == None
    double copies = 0, confidence = 0, mm = 0, pmatch = 0, pindel = 0;
    int64_t max_mm = 0, n_eval = 0, score = 0;
    int64_t req_end = -1;       // the (clamped) end and motif length the recompute
    int32_t req_m = 0;          // was asked for
    int32_t tier = 2;
    char strand = '+';
    bool stats_none = false;    // Rec::stats_none
    // the DP walk stopped at a copy that failed (not at its safety limit):
    // where, and with which min_copies (1: min_copies, 2: the retry with 1).
    // A later call with the same start and motif length whose limit lies past
    // wk_stop walks the same windows (recompute's reuse; refine's calls)
    int8_t wk_phase = 0;
    int64_t wk_stop = -1;
};

static_assert(std::is_trivially_destructible<Extra>::value, "Extras live in raw arena blocks");

// 32 bytes: a strict hit (x == nullptr) is fully determined by its span and
// primitive motif length -- motif = sequence[start, start + mlen) of the frame,
// copies = (end - start) / mlen (bwt.py:1957-1961; also (end - i) / L when the
// unit is primitive), tier 2; every other record carries an Extra
struct Item {
    int64_t start, end;   // current frame (trimmed, then full after restore)
    // recomputed record (nullptr for a strict hit), tagged in bit 0 when its
    // mismatch rate is non-zero: the refine pass tests every fold output and
    // only those records, so it reads no Extra for the others (each read a
    // cache miss: the C3 assembly pass 6.0 -> ~2 ms)
    const Extra *xp;
    int32_t chrom, mlen;
    const Extra *x() const { return reinterpret_cast<const Extra *>(reinterpret_cast<uintptr_t>(xp) & ~uintptr_t(1)); }
    bool imperfect() const { return (reinterpret_cast<uintptr_t>(xp) & 1u) != 0; }
    void set_x(const Extra *e) {   // after e->mm is final
        xp = reinterpret_cast<const Extra *>(reinterpret_cast<uintptr_t>(e) | (e && e->mm != 0.0 ? 1u : 0u));
    }
};
static_assert(sizeof(Item) == 32, "fold items stay 32 bytes");

// vector storage without value-initialisation: large item arrays are written
// once in parallel, so the first touch happens in the filling threads
using ItemVec = std::vector<Item, NoInit<Item>>;

// per-worker bump arenas for Extras and their strings (pointer-stable; the
// blocks are cached huge-page blocks, mem.h)
struct Pools {
    struct Block {
        void *p = nullptr;
        size_t bytes = 0;
        Block(size_t b) : p(big_alloc(b)), bytes(b) {}
        Block(Block &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; }
        Block(const Block &) = delete;
        ~Block() { if (p) big_free(p, bytes); }
    };
    struct Arena {
        std::vector<Block> xb;
        size_t xn = 0;                                   // used in the last Extra block
        std::vector<Block> cb;
        size_t cn = 0, ccap = 0;                         // used / size of the last char block
        // the worker's DP scratch and summary (recompute)
        std::unique_ptr<AlignScratch, void (*)(AlignScratch *)> as{align_scratch_new(), align_scratch_free};
        AlignSummary sum;
        // the last maximal homopolymer run this worker walked: [hlo, hhi) of
        // byte hb in sequence hseq (sequences do not change while the pools live)
        const char *hseq = nullptr;
        int64_t hlo = 0, hhi = 0;
        char hb = 0;
        // the worker's last host recompute whose walk stopped at a copy that
        // failed (not at its safety limit): from the same start with the same
        // motif length, any call whose limit lies past that stop walks the same
        // windows -- a merge chain re-asks this for every record it absorbs
        bool wk_ok = false;
        const char *wk_seq = nullptr;
        int64_t wk_start = 0, wk_m = 0, wk_stop = 0;
        int wk_phase = 0;   // 1: the min_copies walk succeeded; 2: the min_copies = 1 retry
        Item wk_item{};
    };
    static constexpr size_t XB = 16384, CB = size_t(2) << 20;   // Extras are trivially destructible
    std::vector<Arena> a;
    explicit Pools(int n) : a((size_t)n) {}
    std::string_view str(Arena &A, std::string_view s) {
        if (s.empty()) return {};
        if (A.cb.empty() || A.cn + s.size() > A.ccap) {
            A.ccap = std::max(CB, s.size());
            A.cb.emplace_back(A.ccap);
            A.cn = 0;
        }
        char *d = (char *)A.cb.back().p + A.cn;
        std::memcpy(d, s.data(), s.size());
        A.cn += s.size();
        return std::string_view(d, s.size());
    }
    // motif already lives in static storage, no variations
    Extra *add_static(int w, const Extra &e, std::string_view motif) {
        Arena &A = a[(size_t)w];
        if (A.xb.empty() || A.xn == XB) {
            A.xb.emplace_back(XB * sizeof(Extra));
            A.xn = 0;
        }
        Extra *x = (Extra *)A.xb.back().p + A.xn++;
        ::new ((void *)x) Extra(e);
        x->motif = motif;
        x->variations = {};
        return x;
    }
    // a copy of e sharing its strings (the arena keeps them)
    Extra *clone(int w, const Extra &e) {
        Arena &A = a[(size_t)w];
        if (A.xb.empty() || A.xn == XB) {
            A.xb.emplace_back(XB * sizeof(Extra));
            A.xn = 0;
        }
        Extra *x = (Extra *)A.xb.back().p + A.xn++;
        ::new ((void *)x) Extra(e);
        return x;
    }
    Extra *add(int w, const Extra &e, std::string_view motif, std::string_view variations) {
        Arena &A = a[(size_t)w];
        if (A.xb.empty() || A.xn == XB) {
            A.xb.emplace_back(XB * sizeof(Extra));
            A.xn = 0;
        }
        Extra *x = (Extra *)A.xb.back().p + A.xn++;
        ::new ((void *)x) Extra(e);
        x->motif = str(A, motif);
        x->variations = str(A, variations);
        return x;
    }
};

struct UnitCtx {
    const Job *job;
    int64_t min_copies;
    bool restored = false;        // items are in full-sequence coordinates (multi-offset units)
};

inline std::string_view motif_of(const UnitCtx &u, const Item &it) {
    if (it.xp) return it.x()->motif;
    const Contig &c = u.job->contigs[(size_t)it.chrom];
    return std::string_view((u.restored ? c.full.data() : c.trimmed()) + it.start, (size_t)it.mlen);
}
inline int64_t strict_copies(const Item &it) { return (it.end - it.start) / it.mlen; }
inline int32_t tier_of(const Item &it) { return it.xp ? it.x()->tier : 2; }
inline double copies_of(const Item &it) { return it.xp ? it.x()->copies : (double)strict_copies(it); }
inline double mm_of(const Item &it) { return it.xp ? it.x()->mm : 0.0; }
inline double conf_of(const Item &it) { return it.xp ? it.x()->confidence : 0.95; }

// stable sort of items by (start, end)
void sort_by_pos(ItemVec &v, int nt) {
    const size_t n = v.size();
    if (n < 2) return;
    // order checks in parallel chunks (each chunk also checks the pair across its left edge)
    const int C = (int)std::max<size_t>(1, std::min<size_t>((size_t)nt * 4, n / 32768 + 1));
    std::vector<uint8_t> c_sorted((size_t)C, 1), c_start((size_t)C, 1);
    parallel_items(C, nt, [&](int64_t t, int) {
        const size_t a = std::max<size_t>(1, n * (size_t)t / (size_t)C), b = n * (size_t)(t + 1) / (size_t)C;
        bool so = true, bs = true;
        for (size_t i = a; i < b && bs; ++i) {
            bs = v[i - 1].start <= v[i].start;
            so = so && (v[i - 1].start < v[i].start || v[i - 1].end <= v[i].end);
        }
        c_sorted[(size_t)t] = so;
        c_start[(size_t)t] = bs;
    });
    bool sorted = true, by_start = true;
    for (int t = 0; t < C; ++t) {
        sorted = sorted && c_sorted[(size_t)t];
        by_start = by_start && c_start[(size_t)t];
    }
    if (sorted && by_start) return;
    if (by_start) {   // the usual case after merge/refine: only equal-start runs need ordering by end
        // chunk t orders the runs that begin inside it
        parallel_items(C, nt, [&](int64_t t, int) {
            size_t i = n * (size_t)t / (size_t)C;
            const size_t b = n * (size_t)(t + 1) / (size_t)C;
            while (i > 0 && i < b && v[i - 1].start == v[i].start) ++i;
            while (i < b) {
                size_t j = i + 1;
                while (j < n && v[j].start == v[i].start) ++j;
                if (j - i > 1)
                    std::stable_sort(v.begin() + (std::ptrdiff_t)i, v.begin() + (std::ptrdiff_t)j,
                                     [](const Item &x, const Item &y) { return x.end < y.end; });
                i = j;
            }
        });
        return;
    }
    auto lt = [](const Item &a, const Item &b) {
        if (a.start != b.start) return a.start < b.start;
        return a.end < b.end;
    };
    const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)nt, n / 65536 + 1));
    if (T == 1) {
        std::stable_sort(v.begin(), v.end(), lt);
        return;
    }
    std::vector<size_t> cut((size_t)T + 1);
    for (int t = 0; t <= T; ++t) cut[(size_t)t] = n * (size_t)t / (size_t)T;
    parallel_items(T, T, [&](int64_t t, int) { std::stable_sort(v.begin() + cut[(size_t)t], v.begin() + cut[(size_t)t + 1], lt); });
    for (int w = 1; w < T; w *= 2) {    // pairwise stable merges, one level at a time
        std::vector<std::array<size_t, 3>> jobs;
        for (int t = 0; t + w < T; t += 2 * w) jobs.push_back({cut[(size_t)t], cut[(size_t)(t + w)], cut[(size_t)std::min(T, t + 2 * w)]});
        parallel_items((int64_t)jobs.size(), nt, [&](int64_t q, int) {
            auto &j = jobs[(size_t)q];
            std::inplace_merge(v.begin() + j[0], v.begin() + j[1], v.begin() + j[2], lt);
        });
    }
}

// ---------------------------------------------------- nested suppression
// bwt.py:3402-3497.  A repeat is tested only against kept spans of a strictly
// longer motif; the stable sort by (mismatch_rate > 0, -len(motif)) places
// every such span of its class (and the whole perfect class) before it, and
// repeats of equal motif length never test each other.  So each (class,
// length) group is screened -- in parallel, against a frozen grid of the
// spans kept so far -- and its survivors are appended as a whole.  The
// predicate is the reference's, division for division.
ItemVec suppress_nested(const ItemVec &rs, double thr, int nt) {
    const size_t n = rs.size();
    int32_t maxlen = 0;
    for (auto &r : rs) maxlen = std::max(maxlen, r.mlen);
    const size_t nb = 2 * ((size_t)maxlen + 1);
    auto bucket = [&](const Item &r) {
        return (mm_of(r) > 0 ? (size_t)maxlen + 1 : 0) + (size_t)(maxlen - r.mlen);
    };
    std::vector<uint32_t> cnt(nb + 1, 0), order(n);
    for (auto &r : rs) ++cnt[bucket(r) + 1];
    for (size_t b = 0; b < nb; ++b) cnt[b + 1] += cnt[b];
    std::vector<uint32_t> groups(cnt.begin(), cnt.end());
    for (size_t i = 0; i < n; ++i) order[cnt[bucket(rs[i])]++] = (uint32_t)i;

    int64_t maxpos = 1;
    for (auto &r : rs) maxpos = std::max(maxpos, r.end + 1);
    const int64_t B = 256;
    struct Span { int64_t s, e, M; };
    std::vector<std::vector<Span>> grid((size_t)(maxpos / B + 2));
    std::vector<uint8_t> keep(n, 0);
    ItemVec kept;
    kept.reserve(n);
    for (size_t g = 0; g < nb; ++g) {
        const size_t g0 = groups[g], g1 = groups[g + 1];
        if (g0 == g1) continue;
        const bool any_kept = !kept.empty();
        parallel_for((int64_t)(g1 - g0), any_kept ? nt : 1, [&](int64_t a, int64_t b) {
            for (int64_t q = a; q < b; ++q) {
                const Item &r = rs[order[g0 + (size_t)q]];
                const int64_t s0 = r.start, e0 = r.end, m = r.mlen;
                const int64_t rl = e0 - s0;
                bool nested = false;
                if (any_kept && e0 > s0) {
                    const int64_t b0 = std::max<int64_t>(0, s0) / B, b1 = std::max<int64_t>(0, e0 - 1) / B;
                    for (int64_t bk = b0; bk <= b1 && !nested && bk < (int64_t)grid.size(); ++bk) {
                        for (const Span &sp : grid[(size_t)bk]) {
                            if (sp.M <= m) continue;
                            const int64_t ov = std::max<int64_t>(0, std::min(e0, sp.e) - std::max(s0, sp.s));
                            if (ov == 0) continue;
                            const double ratio = (double)sp.M / (double)m;
                            const double frac = (double)ov / (double)rl;
                            if (m == 1 && sp.M > 1 && frac >= 0.8) { nested = true; break; }
                            const double t = ratio >= 10 ? 0.1 : (ratio >= 5 ? 0.3 : thr);
                            if (frac >= t) { nested = true; break; }
                        }
                    }
                }
                keep[order[g0 + (size_t)q]] = !nested;
            }
        });
        for (size_t q = g0; q < g1; ++q) {
            const uint32_t idx = order[q];
            if (!keep[idx]) continue;
            const Item &r = rs[idx];
            if (r.end > r.start) {
                const Span sp{r.start, r.end, (int64_t)r.mlen};
                const int64_t b0 = std::max<int64_t>(0, r.start) / B, b1 = std::max<int64_t>(0, r.end - 1) / B;
                for (int64_t bk = b0; bk <= b1 && bk < (int64_t)grid.size(); ++bk) grid[(size_t)bk].push_back(sp);
            }
            kept.push_back(r);
        }
    }
    return kept;
}

// every byte value as a one-character string (motifs of one-base recomputes)
const struct ByteChars {
    char c[256];
    ByteChars() { for (int i = 0; i < 256; ++i) c[i] = (char)i; }
    const char &operator[](size_t i) const { return c[i]; }
} kByteChars;

inline char comp_of(char c) {   // bwt.py:688-691
    switch (c) {
        case 'A': return 'T';
        case 'T': return 'A';
        case 'C': return 'G';
        case 'G': return 'C';
        default: return c;
    }
}

std::atomic<int64_t> g_recomputes{0}, g_recompute_ns{0}, g_merges{0}, g_canons{0}, g_tests{0}, g_same{0}, g_walk_reuse{0};
// BWTMI_STATS=1: stage timers; =2: also per-recompute / per-test counters (slow)
const char *const g_dump = std::getenv("BWTMI_DUMP_RECOMPUTE");
std::atomic<int64_t> g_hist_n[8][8], g_hist_ns[8][8];
std::atomic<int64_t> g_fresh_tests{0}, g_chain_tests{0}, g_fresh_merges{0}, g_chain_merges{0};   // [log4 motif len][log4 region len]
inline int lg4(int64_t v) { int k = 0; while (v >= 4 && k < 7) { v >>= 2; ++k; } return k; }

// align_repeat_region's result as _recompute_repeat reads it (a host AlignSummary)
struct RcView {
    bool ok = false;
    int64_t consumed = 0, copies = 0, motif_len = 0, max_err = 0, tot_ins = 0, tot_del = 0;
    double mm = 0.0;
    std::string_view consensus, var;
};
Item item_of_alignment(const UnitCtx &u, Pools &pools, int w, int32_t chrom, int64_t start, int64_t end, int64_t m,
                       int32_t tier, std::string_view tmpl, const RcView &v);

// bwt.py:3515-3614 (on the trimmed sequence, before coordinate restore)
// prev (optional): an earlier record from the same start (refine passes the
// record it refines) -- reused when its walk stopped at a failing copy inside
// this call's limit
Item recompute(const UnitCtx &u, Pools &pools, int w, int32_t chrom, int64_t start, int64_t end,
               int64_t motif_len, int32_t tier, const Item *prev = nullptr) {
    struct Tick {   // BWTMI_STATS=2 only
        int a, b;
        std::chrono::steady_clock::time_point t;
        Tick(int a_, int b_) : a(a_), b(b_) { if (stats_on(2)) t = std::chrono::steady_clock::now(); }
        ~Tick() {
            if (!stats_on(2)) return;
            const int64_t ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t).count();
            g_recomputes.fetch_add(1, std::memory_order_relaxed);
            g_recompute_ns.fetch_add(ns, std::memory_order_relaxed);
            g_hist_n[a][b].fetch_add(1, std::memory_order_relaxed);
            g_hist_ns[a][b].fetch_add(ns, std::memory_order_relaxed);
        }
    } tick{lg4(motif_len), lg4(end - start)};
    const Contig &c = u.job->contigs[(size_t)chrom];
    const char *seq = c.trimmed();
    const int64_t L = c.trimmed_len();
    const int64_t m = std::max<int64_t>(1, motif_len);
    start = std::max<int64_t>(0, start);
    end = end > 0 ? std::min(L, end) : L;
    if (end <= start) end = std::min(L, start + m);
    const int64_t req_end = end;
    if (m == 1 && start < L) {
        // One-base motif (~75 % of the recomputes): align_repeat_region's closed
        // form (motif.cpp) without building any strings.  The template is
        // seq[start]; the walk is the run of that base up to its limit, first
        // with min_copies, then (bwt.py:3530-3534) with min_copies 1, which
        // always succeeds (the run holds the template itself).
        const char b = seq[start];
        const int64_t mc = std::max<int64_t>(1, u.min_copies);
        // the maximal run of b through start: a merge chain over one long run
        // (an assembly gap's N run yields a hit per unit length, ~1000 of them,
        // each merge recomputing the union) walks it once per worker
        Pools::Arena &HA = pools.a[(size_t)w];
        if (!(HA.hseq == seq && HA.hb == b && HA.hlo <= start && start < HA.hhi)) {
            HA.hseq = seq;
            HA.hb = b;
            HA.hlo = start;
            HA.hhi = run_end(seq, start, L, b);
        }
        const int64_t hhi = HA.hhi;
        auto run_to = [&](int64_t limit) { return std::min(hhi, limit) - start; };
        int64_t run = run_to(std::min<int64_t>(L, std::max<int64_t>(end, start + mc) + 4));
        if (run < mc) run = run_to(std::min<int64_t>(L, std::max<int64_t>(end, start + 1) + 4));
        Extra x;
        x.copies = (double)run;        // tl / 1 is integral
        x.confidence = 1.0;            // max(0.3, 1 - 0)
        x.mm = 0.0;
        x.n_eval = std::max<int64_t>(1, run);
        x.max_mm = 0;
        const char rc = comp_of(b);
        x.strand = (unsigned char)b <= (unsigned char)rc ? '+' : '-';   // get_canonical_motif_stranded
        x.pmatch = 100.0;
        x.pindel = 0.0;
        x.score = trf_score(run, 0.0);
        x.tier = tier;
        x.req_end = req_end;
        x.req_m = (int32_t)m;
        Item it{};
        it.start = start;
        it.end = start + run;
        it.chrom = chrom;
        it.mlen = 1;
        it.set_x(pools.add_static(w, x, std::string_view(&kByteChars[(uint8_t)b], 1)));
        return it;
    }
    if (g_dump) {   // BWTMI_DUMP_RECOMPUTE=path: the DP recomputes' arguments (tools/recompute_bench.cpp)
        static std::mutex mu;
        std::lock_guard<std::mutex> lk(mu);
        static FILE *df = std::fopen(g_dump, "w");
        if (df) std::fprintf(df, "%lld %lld %lld %lld\n", (long long)start, (long long)end, (long long)m,
                             (long long)std::max<int64_t>(1, u.min_copies));
    }
    auto slice = [&](int64_t a, int64_t b) {   // Python seq[a:b], a,b >= 0
        a = std::min(a, L);
        b = std::min(b, L);
        return b > a ? std::string(seq + a, (size_t)(b - a)) : std::string();
    };
    Pools::Arena &A = pools.a[(size_t)w];
    const int64_t mc = std::max<int64_t>(1, u.min_copies);
    // the walk's safety limit for a min_copies (motif.cpp align_repeat_region, bwt.py:1033)
    const int64_t mi = std::max<int64_t>(1, std::min<int64_t>(10, m >= 4 ? m / 2 : 1));
    auto walk_limit = [&](int64_t mcx) {
        const int64_t e2 = std::min(L, end > start ? end : L);
        return std::min(L, std::max(e2, start + m * mcx) + std::max(m * 3, mi * 4));
    };
    if (prev && prev->xp && prev->start == start && prev->chrom == chrom) {
        const Extra &px = *prev->x();
        if (px.wk_stop >= 0 && px.req_m == m && px.wk_stop < walk_limit(px.wk_phase == 1 ? mc : 1)) {
            if (stats_on(2)) g_walk_reuse.fetch_add(1, std::memory_order_relaxed);
            Extra *x = pools.clone(w, px);
            x->req_end = req_end;
            x->tier = tier;
            Item it = *prev;
            it.set_x(x);
            return it;
        }
    }
    if (A.wk_ok && A.wk_seq == seq && A.wk_start == start && A.wk_m == m &&
        A.wk_stop < walk_limit(A.wk_phase == 1 ? mc : 1)) {
        // the same windows up to the same failing copy: the same record, but
        // for what depends on the call itself (the requested end, the tier)
        if (stats_on(2)) g_walk_reuse.fetch_add(1, std::memory_order_relaxed);
        Extra *x = pools.clone(w, *A.wk_item.x());
        x->req_end = req_end;
        x->tier = tier;
        Item it = A.wk_item;
        it.set_x(x);
        return it;
    }
    std::string tmpl = slice(start, start + m);
    if (tmpl.empty()) {
        const int64_t a = std::max<int64_t>(0, start - m);
        tmpl = slice(a, a + m);
    }
    if (tmpl.empty()) tmpl.assign((size_t)m, 'N');
    AlignSummary &s = A.sum;
    s.want_copies = false;
    int phase = 1;
    // resume: a chain of merges recomputes a growing region from one start,
    // and each walk that stopped at its limit goes on from where it stopped
    constexpr bool resume = true;
    bool ok = align_repeat_region(seq, L, start, end, tmpl, mc, s, 0.1, -1, A.as.get(), resume);
    if (!ok) {
        phase = 2;
        ok = align_repeat_region(seq, L, start, end, tmpl, 1, s, 0.1, -1, A.as.get(), resume);
    }
    RcView v;
    v.ok = ok;
    if (ok) {
        v.consumed = s.consumed;
        v.copies = s.copies;
        v.motif_len = s.motif_len;
        v.max_err = s.max_errors;
        v.tot_ins = s.tot_ins;
        v.tot_del = s.tot_del;
        v.mm = s.mismatch_rate;
        v.consensus = s.consensus;
        if (s.any_variation) v.var = s.variations;
    }
    Item it = item_of_alignment(u, pools, w, chrom, start, end, m, tier, tmpl, v);
    A.wk_ok = ok && !s.at_limit;
    if (A.wk_ok) {   // this worker's new Extra: the record carries its walk's stop for later calls
        Extra *xe = const_cast<Extra *>(it.x());
        xe->wk_stop = start + s.consumed;
        xe->wk_phase = (int8_t)phase;
    }
    if (A.wk_ok) {
        A.wk_seq = seq;
        A.wk_start = start;
        A.wk_m = m;
        A.wk_stop = start + s.consumed;
        A.wk_phase = phase;
        A.wk_item = it;
    }
    return it;
}

// the record _recompute_repeat builds from an alignment (bwt.py:3536-3614)
Item item_of_alignment(const UnitCtx &u, Pools &pools, int w, int32_t chrom, int64_t start, int64_t end, int64_t m,
                       int32_t tier, std::string_view tmpl, const RcView &v) {
    const Contig &c = u.job->contigs[(size_t)chrom];
    const int64_t L = c.trimmed_len();
    const int64_t req_end = end;
    Extra x;
    int64_t consumed, cint;
    double mm, pind;
    std::string_view motif_s = tmpl;   // never empty
    std::string_view var_s;
    if (!v.ok) {
        consumed = std::min(L - start, std::max(m, end - start));
        cint = std::max<int64_t>(1, consumed / m);
        mm = 0.0;
        x.max_mm = 0;
        pind = 0.0;
    } else {
        consumed = v.consumed;
        cint = v.copies;
        if (!v.consensus.empty()) motif_s = v.consensus;
        mm = v.mm;
        const int64_t tb = v.copies * v.motif_len;
        const double ir = tb > 0 ? (double)(v.tot_ins + v.tot_del) / (double)tb : 0.0;
        pind = ir * 100.0;
        x.max_mm = v.max_err;
        var_s = v.var;
    }
    // actual_sequence = sequence[start:start+consumed]
    const int64_t a0 = std::min(start, L), a1 = std::max(a0, std::min(start + consumed, L));
    const int64_t tl = a1 - a0;
    const int64_t mle = (int64_t)motif_s.size();
    double cf = (double)cint;
    if (tl > 0 && mle > 0) {
        const double fr = (double)tl / (double)mle;
        const double rr = std::nearbyint(fr);  // Python round(): half to even
        cf = std::fabs(fr - rr) < 1e-6 ? rr : fr;
    }
    x.copies = cf;
    x.confidence = std::max(0.3, 1.0 - mm);
    x.mm = mm;
    x.n_eval = std::max<int64_t>(1, cint);
    x.strand = canonical_strand(motif_s.data(), (int64_t)motif_s.size());
    x.pmatch = std::max(0.0, 100.0 - mm * 100.0);
    x.pindel = pind;
    x.score = trf_score(tl, mm);
    x.tier = tier;
    x.req_end = req_end;
    x.req_m = (int32_t)m;
    Item it{};
    it.start = start;
    it.end = start + tl;
    it.chrom = chrom;
    it.mlen = (int32_t)motif_s.size();
    it.set_x(pools.add(w, x, motif_s, var_s));
    return it;
}

// ------------------------------------------------------------ merge fold
// bwt.py:3222-3289.  should_merge needs a recompute only for same-canonical
// neighbours within min_len + 1; when it accepts and len(cur.motif) equals the
// min_len it used, _merge_repeats' recompute has identical arguments and that
// result is reused.  Canonical motifs are computed lazily: most neighbours
// fail the distance test first.
struct Canon {
    std::string s;     // canonical string (motifs that do not pack)
    unsigned __int128 key = 0;  // packed canonical word of an ACGT motif <= 64 bases
    int32_t len = -1;  // motif length; -1 = not computed yet
    bool packed = false;
    bool ok = false;
};

// the canonical form of an item's motif, computed once per fold position:
// for ACGT motifs <= 32 bases the least of the packed rotations of the motif
// and of its reverse complement (the packed word orders like the string)
inline void canon_fill(const UnitCtx &u, const Item &it, Canon &c) {
    if (c.ok) return;
    if (stats_on(2)) g_canons.fetch_add(1, std::memory_order_relaxed);
    const std::string_view mv = motif_of(u, it);
    c.len = (int32_t)mv.size();
    uint64_t x;
    c.packed = mv.size() <= 32 && pack2_acgt(mv.data(), (int64_t)mv.size(), x);
    if (c.packed) {
        c.key = canon2(x, (int64_t)mv.size());
    } else if (mv.size() > 32 && mv.size() <= 64 && canon_key128(mv.data(), (int64_t)mv.size(), c.key)) {
        c.packed = true;   // same length on both sides (same_canonical), so the 64- and 128-bit keys never meet
    } else {
        thread_local std::string tmp;
        tmp.assign(mv.data(), mv.size());
        char st;
        canonical_stranded(tmp, c.s, st);
    }
    c.ok = true;
}

// get_canonical_motif_stranded(m1)[0] == ...(m2)[0] (bwt.py:694-716): equal
// canonical forms.  A motif that packs (ACGT only) and one that does not never
// share a canonical form (rotations and the reverse complement keep non-ACGT
// symbols), so mixed pairs are unequal without building strings.
// the canonical form of a one-base motif, by byte (canonical_stranded of that
// byte, computed once per value): at C3 ~3/4 of the merge tests are between
// one-base runs
inline uint8_t canon_base(uint8_t b) {
    static const std::array<uint8_t, 256> t = [] {
        std::array<uint8_t, 256> a{};
        for (int c = 0; c < 256; ++c) {
            std::string cs;
            char st;
            canonical_stranded(std::string(1, (char)c), cs, st);
            a[(size_t)c] = cs.size() == 1 ? (uint8_t)cs[0] : (uint8_t)c;
        }
        return a;
    }();
    return t[b];
}

inline bool same_canonical(const UnitCtx &u, const Item &r1, Canon &c1, const Item &r2, Canon &c2) {
    const int64_t m1 = r1.xp ? (int64_t)r1.x()->motif.size() : r1.mlen, m2 = r2.xp ? (int64_t)r2.x()->motif.size() : r2.mlen;
    if (m1 != m2) return false;
    if (m1 == 0) return true;
    if (m1 == 1)
        return canon_base((uint8_t)motif_of(u, r1)[0]) == canon_base((uint8_t)motif_of(u, r2)[0]);
    canon_fill(u, r1, c1);
    canon_fill(u, r2, c2);
    if (c1.packed != c2.packed) return false;
    return c1.packed ? c1.key == c2.key : c1.s == c2.s;
}


bool try_merge(const UnitCtx &u, Pools &pools, int w, const Item &r1, Canon &c1, const Item &r2, Canon &c2,
               Item &merged) {
    if (r1.chrom != r2.chrom) return false;
    if (r1.mlen == 0 || r2.mlen == 0) return false;
    const int64_t ml = std::min(r1.mlen, r2.mlen);
    if (std::max<int64_t>(0, r2.start - r1.end) > ml + 1) return false;   // cheap test first
    if (stats_on(2)) g_tests.fetch_add(1, std::memory_order_relaxed);
    if (!same_canonical(u, r1, c1, r2, c2)) return false;
    if (stats_on(2)) g_same.fetch_add(1, std::memory_order_relaxed);
    const int64_t s = std::min(r1.start, r2.start), e = std::max(r1.end, r2.end);
    const int32_t tier = std::min(tier_of(r1), tier_of(r2));
    Item mg = recompute(u, pools, w, r1.chrom, s, e, std::max<int64_t>(1, ml), tier);
    if (mg.x()->copies < (double)u.min_copies) return false;
    const double base = std::max(std::max(mm_of(r1), mm_of(r2)), 0.01);
    if (!(mg.x()->mm <= base + 0.2)) return false;
    if (stats_on(2)) g_merges.fetch_add(1, std::memory_order_relaxed);
    if ((int64_t)r1.mlen == std::max<int64_t>(1, ml)) merged = mg;   // len(r1.consensus_motif)
    else merged = recompute(u, pools, w, r1.chrom, s, e, r1.mlen, tier);
    return true;
}

// _refine_repeats (bwt.py:3291-3314) for one record: only recomputed records
// can carry mismatches; a record whose recompute already covered exactly
// [start, end) with this motif length would be recomputed with the same
// arguments (same result)
inline void refine_one(const UnitCtx &u, Pools &pools, int w, Item &r) {
    if (!r.imperfect()) return;   // a strict hit, or mismatch rate 0
    if (r.mlen > 0 && r.mlen == r.x()->req_m && r.x()->req_end == r.end) return;
    int64_t m = r.mlen;
    if (m <= 0) {
        const int64_t rc = (int64_t)std::nearbyint(copies_of(r));
        m = std::max<int64_t>(1, (r.end - r.start) / std::max<int64_t>(1, rc ? rc : 1));
    }
    r = recompute(u, pools, w, r.chrom, r.start, r.end, m, tier_of(r), &r);
}

// bwt.py:3327-3354
bool should_collapse(const UnitCtx &u, const Item &r1, const Item &r2) {
    if (r1.chrom != r2.chrom) return false;
    const int64_t ov = std::min(r1.end, r2.end) - std::max(r1.start, r2.start);
    if (ov <= 0) return false;
    const int64_t sh = std::min(r1.end - r1.start, r2.end - r2.start);
    if (sh <= 0) return false;
    const double f = (double)ov / (double)sh;
    if (f < 0.8) return false;
    {
        Canon c1, c2;
        if (same_canonical(u, r1, c1, r2, c2)) return true;
    }
    if ((r1.mlen == 1 || r2.mlen == 1) && f >= 0.95) return true;
    if (r1.mlen == r2.mlen && f >= 0.9) return std::fabs(mm_of(r1) - mm_of(r2)) >= 0.2;
    return false;
}

// bwt.py:3356-3400 -> true when r1 is preferred
bool prefer_first(const UnitCtx &u, const Item &r1, const Item &r2) {
    const std::string_view m1 = motif_of(u, r1), m2 = motif_of(u, r2);
    const size_t l1 = m1.size(), l2 = m2.size();
    if (l1 != l2) {
        if (l1 == 1 && l2 > 1) return false;
        if (l2 == 1 && l1 > 1) return true;
        const std::string_view sh = l1 < l2 ? m1 : m2, lo = l1 < l2 ? m2 : m1;
        if (lo.size() % sh.size() == 0) {
            bool rep = true;
            for (size_t i = 0; i < lo.size() && rep; ++i) rep = lo[i] == sh[i % sh.size()];
            if (rep) return l1 < l2;
        }
        return l1 > l2;
    }
    if (mm_of(r1) != mm_of(r2)) return mm_of(r1) < mm_of(r2);
    if (conf_of(r1) != conf_of(r2)) return conf_of(r1) > conf_of(r2);
    const int64_t len1 = r1.end - r1.start, len2 = r2.end - r2.start;
    if (len1 != len2) return len1 >= len2;
    return true;
}

// bwt.py:3189-3220.  After the (start, end) sort, equal keys (chrom, start,
// end, motif) sit inside runs of equal (start, end); the first occurrence
// keeps its position and takes the preferred content.
void dedup_sorted(const UnitCtx &u, ItemVec &recs) {
    ItemVec d;
    d.reserve(recs.size());
    size_t i = 0;
    const size_t n = recs.size();
    while (i < n) {
        size_t j = i + 1;
        while (j < n && recs[j].start == recs[i].start && recs[j].end == recs[i].end) ++j;
        const size_t first_out = d.size();
        for (size_t q = i; q < j; ++q) {
            const Item &r = recs[q];
            size_t hit = SIZE_MAX;
            for (size_t x = first_out; x < d.size(); ++x)
                if (d[x].chrom == r.chrom && d[x].mlen == r.mlen && motif_of(u, d[x]) == motif_of(u, r)) {
                    hit = x;
                    break;
                }
            if (hit == SIZE_MAX) { d.push_back(r); continue; }
            const Item &ex = d[hit];
            bool repl = false;
            if (conf_of(r) > conf_of(ex)) repl = true;
            else if (conf_of(r) == conf_of(ex)) {
                if (mm_of(r) < mm_of(ex)) repl = true;
                else if (mm_of(r) == mm_of(ex) && tier_of(r) < tier_of(ex)) repl = true;
            }
            if (repl) d[hit] = r;
        }
        i = j;
    }
    recs.swap(d);
}

// an input record that is not a strict hit (Tier 3): every field carried in an Extra
Item item_of_rec(Pools &pools, const Rec &r) {
    Extra x;
    x.copies = r.copies;
    x.confidence = r.confidence;
    x.mm = r.mismatch_rate;
    x.pmatch = r.pmatch;
    x.pindel = r.pindel;
    x.max_mm = r.max_mm;
    x.n_eval = r.n_eval;
    x.score = r.score;
    x.strand = r.strand;
    x.stats_none = r.stats_none;
    x.tier = r.tier;
    Item it{};
    it.start = r.start;
    it.end = r.end;
    it.chrom = r.chrom;
    it.mlen = (int32_t)r.motif.size();
    it.set_x(pools.add(0, x, r.motif, r.variations));
    return it;
}

// final Rec of an item (after restore): strict fields per bwt.py:1972-1993
void materialize(const UnitCtx &u, const Item &it, int64_t shift, Rec &r) {   // r: a fresh Rec
    const Contig &c = u.job->contigs[(size_t)it.chrom];
    r.chrom = it.chrom;
    r.tier = tier_of(it);
    r.start = it.start + shift;
    r.end = it.end + shift;
    r.length = it.end - it.start;
    if (it.xp) {
        const Extra &x = *it.x();
        r.motif = x.motif;
        r.copies = x.copies;
        r.confidence = x.confidence;
        r.mismatch_rate = x.mm;
        r.max_mm = x.max_mm;
        r.n_eval = x.n_eval;
        r.strand = x.strand;
        r.pmatch = x.pmatch;
        r.pindel = x.pindel;
        r.score = x.score;
        r.variations = x.variations;
        r.stats_none = x.stats_none;
    } else {
        r.motif.assign(c.trimmed() + (it.start - (u.restored ? c.trim_left : 0)), (size_t)it.mlen);
        const int64_t count = strict_copies(it);
        r.copies = (double)count;
        r.confidence = 0.95;
        r.mismatch_rate = 0.0;
        r.max_mm = 0;
        r.n_eval = count;
        r.strand = '+';
        r.pmatch = (1.0 - 0.0) * 100.0;
        r.pindel = 0.0;
        r.score = trf_score(r.length, 0.0);
    }
    // actual_sequence = full_sequence[start:end] after restore (bwt.py:3323-3325)
    if (!c.full.empty()) {
        const int64_t L = (int64_t)c.full.size();
        const int64_t a = std::min(r.start, L), b = std::max(a, std::min(r.end, L));
        r.act_kind = ACT_FULL;
        r.act_off = a;
        r.act_len = b - a;
    }
}

// ------------------------------------------------- one pass over cut segments
// For a unit of one contig whose input records are all strict hits, in
// (start, end) order, hit k is a CUT (fold_cut, common.h) when
//   S[k] - max_{j < k} reach(j) > max(1, M[k]) + 1,
// reach(j) (screen_reach) being how far a record built from hit j and hits
// after it is expected to end: by a merge, a chain of merges, or the refine of
// such a record.  Where every record from before hit k does end at most at
// R = max reach(j),
//   * the fold restarts.  The record the fold holds when hit k arrives was
//     built from earlier hits; the merge test asks for a gap of at most
//     min(mlen) + 1, and min(mlen) + 1 <= M[k] + 1 because hit k's own motif
//     length is one of the two: the test fails, the record is emitted and hit k
//     becomes the current record, fresh.  Every earlier record has been emitted
//     by then, and the fold only ever looks at its current record: what it does
//     from k on does not depend on anything before k;
//   * the collapse restarts.  It compares a record with the last one it kept,
//     and collapsing needs an overlap.  Every record from before the cut ends
//     (refined or not) at most at R < S[k], every record from k on starts at
//     S[k] or later (a merged record starts where its first hit did);
//   * the (start, end) order holds across the cut: a record ends after it
//     starts, so every start before the cut is < S[k] <= every start after it,
//     and the equal-start runs that the refine can put out of order lie inside
//     segments;
//   * hits that the device screen dropped only loosen the bound.  Its R runs
//     over every kept hit before the drop, a superset of the hits folded here,
//     so R is at least the maximum over the hits that are left.
// So the segments between consecutive cuts are independent from the fold to
// the final filter (bwt.py:3222-3289, 3291-3314, 3499-3513, 3940-3944), and a
// task runs all of it on one segment at a time, while its records are in
// cache, and keeps only the survivors.  Nothing is speculated.
//
// reach() is the recompute's walk limit, and the walk's last copy starts before
// that limit but may end up to m + max_indel - 1 past it (motif.cpp); a chain of
// merges can also carry a walk on from where the last one stopped.  So a bit is
// taken as a hint, and a cut is USED only once it is verified on the records
// themselves: the fold runs its ordinary merge test at hit k, and the segment
// is closed there only if that test failed and every record of the segment,
// after its refine, ends at most at S[k] - max(1, M[k]) - 2 -- the three points
// above with the real ends in place of R.  An unverified bit is an ordinary
// hit.  A task that finds the bit at its end unverified folds on to the next
// verified cut; the tasks it ran through are folded again from there, serially
// (reconcile below; rare: on a 200 kbp contig with 2 % substitutions one bit
// in ~8000 fails, and only one at a task's edge costs anything).
//
// Every fold unit takes this pass.  The bound says nothing about a unit of
// several contigs (their records interleave by position) or about records that
// carry an Extra on input (Tier 3), and BWTMI_FOLD_CUTS=0 asks for the answer
// without cuts: such a source has no bits, record 0 opens the one segment, and
// that segment gets the reference's serial fold, refine, order, collapse and
// filter on one thread.
struct CutSrc {
    const ScreenedVec *sh = nullptr;   // device-screened hits (bits: use theirs), or
    bool bits = true;
    const ItemVec *recs = nullptr;     // gathered records and their bits (cut == nullptr: none)
    const uint8_t *cut = nullptr;
    int32_t chrom = 0;
    int64_t n = 0;
    bool has_bits() const { return sh ? bits : cut != nullptr; }
    void wait(int64_t k) const {   // records [0, k) readable
        if (sh) sh->wait(std::min(k, n));
    }
    bool get(int64_t k, Item &it) const {   // record k; true: a cut (record 0 always opens a segment)
        if (sh) {
            int64_t s0, len, prim;
            const bool c = sh->get(k, s0, len, prim);
            it = Item{s0, s0 + len, nullptr, chrom, (int32_t)prim};
            return (c && bits) || k == 0;   // (the screen may have dropped the hits before the first one)
        }
        it = (*recs)[(size_t)k];
        return k == 0 || (cut && cut[k] != 0);
    }
};

// the cut bits of n strict hits in (start, end) order, at(k, s, e, m): the
// largest reach per chunk in parallel, a prefix over the chunks, a sequential
// prefix inside each chunk
template <class At>
std::vector<uint8_t> host_cuts(int64_t n, int64_t min_copies, bool unit1_maximal, int nt, At &&at) {
    std::vector<uint8_t> cut((size_t)n);
    const int32_t mc = (int32_t)std::max<int64_t>(1, std::min<int64_t>(min_copies, INT32_MAX));
    const int C = n > 8192 ? 4 * std::max(1, nt) : 1;
    std::vector<int64_t> cmax((size_t)C, INT64_MIN), pre((size_t)C, INT64_MIN);
    auto reach = [&](int64_t k) {
        int64_t s, e, m;
        at(k, s, e, m);
        return screen_reach(s, e, std::max<int64_t>(1, m), mc, unit1_maximal);
    };
    if (C > 1)
        parallel_items(C, nt, [&](int64_t t, int) {
            int64_t r = INT64_MIN;
            for (int64_t k = n * t / C; k < n * (t + 1) / C; ++k) r = std::max(r, reach(k));
            cmax[(size_t)t] = r;
        });
    for (int t = 1; t < C; ++t) pre[(size_t)t] = std::max(pre[(size_t)t - 1], cmax[(size_t)t - 1]);
    parallel_items(C, nt, [&](int64_t t, int) {
        int64_t r = pre[(size_t)t];
        for (int64_t k = n * t / C; k < n * (t + 1) / C; ++k) {
            int64_t s, e, m;
            at(k, s, e, m);
            cut[(size_t)k] = fold_cut(s, m, r);
            r = std::max(r, reach(k));
        }
    });
    return cut;
}

// BWTMI_DEVICE_CHECKS=1: the device's cut bits against the host's.  Without
// the drop they are equal; with it the device's bound also covers the dropped
// hits, so it may only be the stricter one (a device cut is a host cut).
void check_device_cuts(const UnitCtx &u, const ScreenedVec &sh, int nt) {
    const int64_t n = sh.size();
    sh.wait(n);
    const std::vector<uint8_t> hc = host_cuts(n, u.min_copies, true, nt, [&](int64_t k, int64_t &s, int64_t &e, int64_t &m) {
        int64_t len;
        (void)sh.get(k, s, len, m);
        e = s + len;
    });
    for (int64_t k = 0; k < n; ++k) {
        int64_t s, len, m;
        const bool d = sh.get(k, s, len, m);
        if (sh.dropped ? d && !hc[(size_t)k] : d != (hc[(size_t)k] != 0))
            fail(BWTMI_E_STATE, "cut bit of screened hit %lld (start %lld, unit %lld): device %d, host %d", (long long)k,
                 (long long)s, (long long)m, (int)d, (int)hc[(size_t)k]);
    }
}

// The fused pass.  Tasks are nominal chunks of records (BWTMI_FOLD_CHUNK
// records each; 0: at most 8 tasks per thread and at least 2048 records each),
// claimed in ascending order; task k owns the records from the first cut at or
// after its nominal start up to the first cut at or after its nominal end
// (none in its range: nothing), and waits for the download of those records
// only.
// The survivors go to `out` in order, as Items: nobody on the path from a FASTA
// to a file reads a Rec, so none is built here (SurvivorSet below).
// `shift` is the unit's common trim offset, added when the survivors are
// viewed or materialised: the (start, end) order is unchanged by it and collapse only
// compares overlaps, lengths and motifs.  restore: the unit's contigs have
// different trim offsets (one of them is <= 2 trim long, offset 0), so its
// segment goes to full-sequence coordinates before the collapse, as in
// bwt.py:3316-3325, and shift is 0; such a unit has several contigs, so no bits.
void fold_cuts(UnitCtx u, Pools &pools, const CutSrc &src, int nt, int64_t shift, bool restore, ItemVec &out, double *ms) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    const int64_t n = src.n;
    if (n == 0) return;
    if (restore && (src.has_bits() || shift != 0)) fail(BWTMI_E_STATE, "cut bits or a common shift on a unit with several trim offsets");
    const int64_t chunk = std::max<int64_t>(0, knob(KN_FOLD_CHUNK));
    const int64_t K = chunk > 0 ? (n + chunk - 1) / chunk : std::max<int64_t>(1, std::min<int64_t>((int64_t)nt * 8, n / 2048 + 1));
    auto nom = [&](int64_t k) { return chunk > 0 ? std::min(n, k * chunk) : n * k / K; };
    // test hook: BWTMI_FAIL_MERGE_CHUNK=k throws inside task k (-2: the last task)
    const int64_t inj_k = knob(KN_FAIL_MERGE_CHUNK);
    const int64_t inj = inj_k == -1 ? -1 : inj_k < 0 ? K - 1 : inj_k;
    const double mcd = (double)u.job->params.min_copies;
    // per task: the records that pass the final filter (slot K: a tail the reconcile folds)
    std::vector<std::vector<Item>> surv((size_t)K + 1);
    std::vector<int64_t> first((size_t)K, -1), stop((size_t)K, -1);   // the range a task folded: [first, stop)
    std::vector<double> cms(stats_on() ? (size_t)K : 0);
    std::atomic<int64_t> n_cuts{0}, n_unverified{0}, n_folded{0}, n_collapsed{0};
    auto lt = [](const Item &a, const Item &b) { return a.start != b.start ? a.start < b.start : a.end < b.end; };
    // the fold from record i (a verified cut, or 0) to the first verified cut at
    // or after ne (returned; n: the end), survivors appended to sv
    auto fold_range = [&](int64_t i, int64_t ne, int w, std::vector<Item> &sv) -> int64_t {
        std::vector<Item> seg;   // the fold's output since the last verified cut
        size_t refined = 0;      // seg[0, refined) have been through refine
        int64_t mx = INT64_MIN;  // the largest end in seg, before or after refine
        int64_t cuts = 1, unverified = 0, folded = 0, collapsed = 0, waited = 0;
        auto refine_seg = [&] {
            for (; refined < seg.size(); ++refined) {
                Item &it = seg[refined];
                mx = std::max(mx, it.end);
                if (it.imperfect()) {
                    refine_one(u, pools, w, it);
                    mx = std::max(mx, it.end);
                }
            }
        };
        // order, collapse and filter the (refined) segment
        auto close_seg = [&] {
            // the fold's output is ordered by start and refine only moves ends:
            // equal-start runs go by end (any other disorder: the same stable sort)
            if (!std::is_sorted(seg.begin(), seg.end(), lt)) std::stable_sort(seg.begin(), seg.end(), lt);
            if (restore) {   // the one segment: each record to its contig's full frame, ordered again (bwt.py:3316-3325, 3505)
                for (Item &it : seg) {
                    const int64_t off = u.job->contigs[(size_t)it.chrom].trim_left;
                    it.start += off;
                    it.end += off;
                }
                u.restored = true;   // motif_of and materialize read the full sequence from here on
                std::stable_sort(seg.begin(), seg.end(), lt);
            }
            folded += (int64_t)seg.size();
            auto emit = [&](const Item &x) {
                ++collapsed;
                if (copies_of(x) >= mcd && x.end - x.start >= 6) sv.push_back(x);
            };
            Item last = seg[0];   // the slot takes the preferred record
            for (size_t q = 1; q < seg.size(); ++q) {
                if (should_collapse(u, last, seg[q])) {
                    if (!prefer_first(u, last, seg[q])) last = seg[q];
                } else {
                    emit(last);
                    last = seg[q];
                }
            }
            emit(last);
            seg.clear();
            refined = 0;
            mx = INT64_MIN;
        };
        Item cur, r, mg;
        src.wait(waited = std::min(n, std::max(ne, i + 1)));
        (void)src.get(i, cur);
        Canon cb[2];   // canonical forms of cur and of the next record; roles swap by index
        int ci_cur = 0;
        bool merged = false;   // cur is the result of a merge (BWTMI_STATS=2 counts the steps by it)
        int64_t j = i + 1;
        for (; j < n; ++j) {
            if (j >= waited) src.wait(waited = std::min(n, j + 256));   // past the nominal end, up to the next cut
            const bool bit = src.get(j, r);
            Canon &cc = cb[ci_cur], &ci = cb[ci_cur ^ 1];
            ci.ok = false;
            if (stats_on(2)) (merged ? g_chain_tests : g_fresh_tests).fetch_add(1, std::memory_order_relaxed);
            if (try_merge(u, pools, w, cur, cc, r, ci, mg)) {
                if (stats_on(2)) (merged ? g_chain_merges : g_fresh_merges).fetch_add(1, std::memory_order_relaxed);
                cur = mg;
                merged = true;
                cc.ok = false;
                unverified += bit;
                continue;
            }
            seg.push_back(cur);
            cur = r;
            merged = false;
            ci_cur ^= 1;
            if (!bit) continue;
            refine_seg();
            if (!fold_cut(r.start, r.mlen, mx)) {
                ++unverified;
                continue;
            }
            close_seg();
            if (j >= ne) break;
            ++cuts;
        }
        if (j >= n) {   // the end of the records closes the last segment
            seg.push_back(cur);
            refine_seg();
            close_seg();
            j = n;
        }
        n_cuts.fetch_add(cuts, std::memory_order_relaxed);
        n_unverified.fetch_add(unverified, std::memory_order_relaxed);
        n_folded.fetch_add(folded, std::memory_order_relaxed);
        n_collapsed.fetch_add(collapsed, std::memory_order_relaxed);
        return j;
    };
    auto task = [&](int64_t k, int w) {
        if (k == inj) fail(BWTMI_E_STATE, "injected failure in merge task %lld", (long long)k);
        const auto a = clk::now();
        const int64_t ne = nom(k + 1);
        src.wait(ne);
        int64_t i = nom(k);
        Item r;
        while (i < ne && !src.get(i, r)) ++i;
        if (i >= ne) return;   // no cut in the range: an earlier task folds through it
        first[(size_t)k] = i;
        stop[(size_t)k] = fold_range(i, ne, w, surv[(size_t)k]);
        if (stats_on()) cms[(size_t)k] = std::chrono::duration<double, std::milli>(clk::now() - a).count();
    };
    int64_t redone = 0;
    {
        BWTMI_STAGE("bwtmi:merge");
        parallel_items(K, nt, task);   // dynamic: the tasks' costs are uneven
        // reconcile: a task whose start the fold before it ran through (the bit
        // there was not verified) is folded again from where that fold stopped
        int64_t pos = 0;
        for (int64_t k = 0; k < K; ++k) {
            if (first[(size_t)k] < 0 || first[(size_t)k] == pos) {
                if (first[(size_t)k] >= 0) pos = stop[(size_t)k];
                continue;
            }
            surv[(size_t)k].clear();
            ++redone;
            if (pos < nom(k + 1)) pos = fold_range(pos, nom(k + 1), 0, surv[(size_t)k]);
        }
        if (pos < n) {
            (void)fold_range(pos, n, 0, surv[(size_t)K]);
            ++redone;
        }
    }
    const auto t1 = clk::now();
    // the tasks' survivors, in order, in one array
    BWTMI_STAGE("bwtmi:refine..filter");
    const int64_t KS = K + 1;
    std::vector<int64_t> cnt((size_t)KS + 1, 0);
    for (int64_t k = 0; k < KS; ++k) cnt[(size_t)k + 1] = cnt[(size_t)k] + (int64_t)surv[(size_t)k].size();
    out.resize((size_t)cnt[(size_t)KS]);
    parallel_items(KS, nt, [&](int64_t t, int) {
        std::copy(surv[(size_t)t].begin(), surv[(size_t)t].end(), out.begin() + (std::ptrdiff_t)cnt[(size_t)t]);
    });
    const auto t2 = clk::now();
    auto d = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    if (stats_on()) {
        double sum = 0, mx = 0;
        for (double v : cms) { sum += v; mx = std::max(mx, v); }
        std::fprintf(stderr, "  merge+refine+collapse+filter in one pass %.1f ms (K=%lld, task sum %.1f max %.1f ms): %lld hits, "
                     "%lld cuts (%lld bits unverified, %lld tasks folded again), merge -> %lld, collapse -> %lld, "
                     "filter -> %lld; survivors gathered in %.1f ms\n",
                     d(t0, t1), (long long)K, sum, mx, (long long)n, (long long)n_cuts.load(), (long long)n_unverified.load(),
                     (long long)redone, (long long)n_folded.load(), (long long)n_collapsed.load(), (long long)cnt[(size_t)KS],
                     d(t1, t2));
    }
    if (ms) {
        ms[2] += d(t0, t2);
    }
}

// a fold unit's final records: the fold's survivors in (start, end) order, the
// arenas their Extras and strings live in, and the frame they are in
struct UnitRes {
    ItemVec items;
    std::unique_ptr<Pools> pools;
    int64_t shift = 0;       // added to every position (the unit's common trim offset)
    bool restored = false;   // positions are full-sequence ones already
    int32_t unit = 0, contigs = 0;
};

void process_unit(const Job &job, const std::vector<int32_t> &chroms, std::vector<HitVec> &raw,
                  std::vector<ScreenedVec> &shits, UnitRes &res, double *ms, int nt) {
    using clk = std::chrono::steady_clock;
    auto t0 = clk::now();
    UnitCtx u{&job, job.params.min_copies};
    res.pools = std::make_unique<Pools>(std::max(1, nt));
    Pools &pools = *res.pools;
    ItemVec &out = res.items;
    // Every unit ends in fold_cuts, the fold to the filter in one pass.  Cut
    // bits are used (BWTMI_FOLD_CUTS, default 1) where screen_reach bounds the
    // records: one contig, strict hits only.  Anything else is one segment.
    const bool cuts_on = knob(KN_FOLD_CUTS) != 0 && chroms.size() == 1;
    // With one trim offset for the whole unit the records keep their trimmed
    // coordinates to the end and the offset is added when they are materialised;
    // with several, fold_cuts restores them before the collapse.
    bool one_offset = true;
    for (int32_t c : chroms) one_offset = one_offset && job.contigs[(size_t)c].trim_left == job.contigs[(size_t)chroms[0]].trim_left;
    const int64_t shift = one_offset && !chroms.empty() ? job.contigs[(size_t)chroms[0]].trim_left : 0;
    res.shift = shift;
    res.restored = !one_offset;   // fold_cuts restores such a unit's one segment before the collapse
    res.contigs = (int32_t)chroms.size();
    auto d = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    // one device-screened contig without Tier 3 records (the usual unit): the
    // tasks of the pass read its compact hits, which never enter a shared array
    if (chroms.size() == 1) {
        const int32_t c = chroms[0];
        const bool scr = (size_t)c < job.screened.size() && job.screened[(size_t)c] && (size_t)c < shits.size();
        const bool mine = job.selected.empty() || ((size_t)c < job.selected.size() && job.selected[(size_t)c]);
        const bool t3 = mine && (size_t)c < job.t3.size() && !job.t3[(size_t)c].empty();
        if (scr && !t3) {
            const ScreenedVec &sh = shits[(size_t)c];
            if (cuts_on && knob(KN_DEVICE_CHECKS)) check_device_cuts(u, sh, nt);
            CutSrc src;
            src.sh = &sh;
            src.bits = cuts_on;
            src.chrom = c;
            src.n = sh.size();
            auto t1 = clk::now();
            fold_cuts(u, pools, src, nt, shift, false, out, ms);
            ScreenedVec().swap(shits[(size_t)c]);
            HitVec().swap(raw[(size_t)c]);
            if (ms) ms[0] += d(t0, t1);
            return;
        }
    }
    // 1. nested suppression per chromosome (bwt.py:3928), concatenated in
    //    chromosome order, stable-sorted by (start, end).
    //    Hits the device already screened (nested.hip) arrive kept, sorted and
    //    deduplicated per chromosome; a one-chromosome unit then skips the sort
    //    and the dedup.
    ItemVec recs;
    bool presorted = chroms.size() == 1;
    bool strict_only = true;   // no input record carries an Extra
    for (int32_t c : chroms) {
        auto &h = raw[(size_t)c];
        const bool scr = (size_t)c < job.screened.size() && job.screened[(size_t)c];
        presorted = presorted && scr;
        ItemVec items;
        if (scr && (size_t)c < shits.size()) {   // device-screened: compact records
            auto &sh = shits[(size_t)c];
            items.resize(sh.size());
            sh.wait(sh.size());
            parallel_for((int64_t)sh.size(), nt, [&](int64_t a, int64_t b) {
                for (int64_t k = a; k < b; ++k) {
                    int64_t s0, len, prim;
                    sh.get(k, s0, len, prim);
                    items[(size_t)k] = Item{s0, s0 + len, nullptr, c, (int32_t)prim};
                }
            });
            ScreenedVec().swap(sh);
        } else {
            items.resize(h.size());
            parallel_for((int64_t)h.size(), nt, [&](int64_t a, int64_t b) {
                for (int64_t k = a; k < b; ++k) {
                    const bwtmi_hit &x = h[(size_t)k];
                    items[(size_t)k] = Item{x.start, x.end, nullptr, c, x.prim_len};
                }
            });
        }
        HitVec().swap(h);
        // Tier 3 records of this chromosome come after all worker records (bwt.py:3918-3924)
        const bool mine = job.selected.empty() || ((size_t)c < job.selected.size() && job.selected[(size_t)c]);
        if (mine && (size_t)c < job.t3.size() && !job.t3[(size_t)c].empty()) {
            if (scr) fail(BWTMI_E_STATE, "contig %d holds device-screened hits and Tier 3 records", (int)c);
            for (const Rec &r : job.t3[(size_t)c]) items.push_back(item_of_rec(pools, r));
            strict_only = false;
        }
        if (!scr) items = suppress_nested(items, 0.5, nt);
        if (recs.empty()) recs.swap(items);
        else recs.insert(recs.end(), items.begin(), items.end());
    }
    if (!presorted) sort_by_pos(recs, nt);
    auto t1 = clk::now();
    // 2. dedup (bwt.py:3189-3220)
    if (!presorted) dedup_sorted(u, recs);
    auto t2 = clk::now();
    // 3. the cut bits of host-screened strict hits, then merge, refine, restore,
    //    collapse and the final filter in the one pass
    std::vector<uint8_t> cut;
    if (cuts_on && strict_only)
        cut = host_cuts((int64_t)recs.size(), u.min_copies, false, nt, [&](int64_t k, int64_t &s, int64_t &e, int64_t &m) {
            const Item &r = recs[(size_t)k];
            s = r.start;
            e = r.end;
            m = r.mlen;
        });
    CutSrc src;
    src.recs = &recs;
    src.cut = cut.empty() ? nullptr : cut.data();
    src.n = (int64_t)recs.size();
    const auto t_bits = clk::now();
    fold_cuts(u, pools, src, nt, shift, !one_offset, out, ms);
    if (ms) {
        ms[0] += d(t0, t1);
        ms[1] += d(t1, t2);
        ms[2] += d(t2, t_bits);   // the cut bits
    }
}

// The units' survivors as the job keeps them (common.h Survivors).  view() and
// materialize() state the same record: strict fields per bwt.py:1972-1993,
// recomputed ones from their Extra.
struct SurvivorSet final : Survivors {
    const Job *job = nullptr;
    std::vector<UnitRes> us;   // units with records, in unit order
    size_t total = 0;
    size_t size() const override { return total; }
    size_t units() const override { return us.size(); }
    int32_t unit_id(size_t k) const override { return us[k].unit; }
    int32_t unit_chrom(size_t k) const override { return us[k].items[0].chrom; }
    size_t unit_size(size_t k) const override { return us[k].items.size(); }
    void span(size_t k, size_t i, int64_t &start, int64_t &end, int32_t &mlen) const override {
        const Item &it = us[k].items[i];
        start = it.start + us[k].shift;
        end = it.end + us[k].shift;
        mlen = it.mlen;   // every Item's mlen is its motif's length (strict: the primitive unit; recomputed: its Extra's motif)
    }
    RecRef view(size_t k, size_t i) const override {
        const UnitRes &U = us[k];
        const Item &it = U.items[i];
        const Contig &c = job->contigs[(size_t)it.chrom];
        RecRef v;
        v.chrom = it.chrom;
        v.tier = tier_of(it);
        v.start = it.start + U.shift;
        v.end = it.end + U.shift;
        if (it.xp) {
            const Extra &x = *it.x();
            v.motif = x.motif.data();
            v.mlen = (int32_t)x.motif.size();
            v.copies = x.copies;
            v.confidence = x.confidence;
            v.mismatch_rate = x.mm;
            v.max_mm = x.max_mm;
            v.n_eval = x.n_eval;
            v.strand = x.strand;
            v.pmatch = x.pmatch;
            v.pindel = x.pindel;
            v.score = x.score;
            v.var = x.variations.data();
            v.vlen = (int32_t)x.variations.size();
            v.stats_none = x.stats_none;
        } else {
            v.motif = c.trimmed() + (it.start - (U.restored ? c.trim_left : 0));
            v.mlen = it.mlen;
            const int64_t count = strict_copies(it);
            v.copies = (double)count;
            v.confidence = 0.95;
            v.mismatch_rate = 0.0;
            v.max_mm = 0;
            v.n_eval = count;
            v.strand = '+';
            v.pmatch = (1.0 - 0.0) * 100.0;
            v.pindel = 0.0;
            v.score = trf_score(it.end - it.start, 0.0);
        }
        // actual_sequence = full_sequence[start:end] after restore (bwt.py:3323-3325)
        if (!c.full.empty()) {
            const int64_t L = (int64_t)c.full.size();
            const int64_t a = std::min(v.start, L), b = std::max(a, std::min(v.end, L));
            v.act = c.full.data() + a;
            v.act_len = b - a;
        }
        return v;
    }
    // Every slot is constructed whatever throws: a task whose materialize
    // throws constructs the rest of its slots before it reports, and the tasks
    // after it only construct theirs, so the vector's destructor never meets a
    // raw slot.
    void materialize(RecVec &out, int nt) const override {
        struct Task { size_t k, a, b, o; };
        std::vector<Task> tasks;
        size_t o = 0;
        for (size_t k = 0; k < us.size(); ++k)
            for (size_t a = 0, n = us[k].items.size(); a < n; a += 4096) {
                tasks.push_back({k, a, std::min(n, a + 4096), o});
                o += std::min(n, a + 4096) - a;
            }
        {
            DeferConstruct raw;   // constructed below, in parallel
            out.resize(total);
        }
        static_assert(std::is_nothrow_default_constructible<Rec>::value, "Rec() must not throw");
        // test hook: BWTMI_FAIL_MATERIALISE != 0 throws inside the last task
        const bool inject = knob(KN_FAIL_MATERIALISE) != 0;
        std::atomic<bool> failed{false};
        std::exception_ptr err;
        std::mutex err_mu;
        parallel_items((int64_t)tasks.size(), nt, [&](int64_t t, int) {
            const Task &T = tasks[(size_t)t];
            const UnitRes &U = us[T.k];
            UnitCtx u{job, job->params.min_copies};
            u.restored = U.restored;
            size_t q = T.o;   // slots [T.o, q) are constructed
            const size_t q1 = T.o + (T.b - T.a);
            if (!failed.load(std::memory_order_relaxed)) {
                try {
                    for (size_t j = T.a; j < T.b; ++j) {
                        if (j + 8 < T.b && U.items[j + 8].xp) __builtin_prefetch(U.items[j + 8].x());
                        ::new ((void *)&out[q]) Rec();
                        ++q;
                        bwtmi::materialize(u, U.items[j], U.shift, out[q - 1]);
                    }
                    if (inject && (size_t)t + 1 == tasks.size()) fail(BWTMI_E_STATE, "injected failure building the records");
                } catch (...) {
                    failed.store(true, std::memory_order_relaxed);
                    std::lock_guard<std::mutex> lk(err_mu);
                    if (!err) err = std::current_exception();
                }
            }
            for (; q < q1; ++q) ::new ((void *)&out[q]) Rec();
        });
        if (err) std::rethrow_exception(err);
    }
};

}  // namespace

// The records are built from the survivors by the first reader that asks for
// them; two threads may ask at once.  A failure leaves them pending.
RecVec &Job::recs() {
    std::lock_guard<std::mutex> lk(recs_mu);
    if (recs_pending) {
        RecVec built;
        surv->materialize(built, host_threads(params));
        final_recs.swap(built);
        recs_pending = false;
    }
    return final_recs;
}

RecVec &Job::recs_own() {
    RecVec &r = recs();
    std::shared_ptr<Survivors> old;
    {
        std::lock_guard<std::mutex> lk(recs_mu);
        old.swap(surv);
    }
    if (old) defer([old]() mutable { old.reset(); });
    return r;
}

size_t Job::count() const {
    std::lock_guard<std::mutex> lk(recs_mu);
    return recs_pending ? surv->size() : final_recs.size();
}

std::shared_ptr<Survivors> Job::survivors() const {
    std::lock_guard<std::mutex> lk(recs_mu);
    return surv;
}

void Job::keep_survivors(std::shared_ptr<Survivors> s) {
    std::lock_guard<std::mutex> lk(recs_mu);
    surv = std::move(s);
    recs_pending = true;
}

void Job::drop_results() {
    std::lock_guard<std::mutex> lk(recs_mu);
    recs_pending = false;
    // released on the background reaper thread, behind the next step's device phase
    auto old_s = std::make_shared<std::shared_ptr<Survivors>>(std::move(surv));
    surv = nullptr;
    auto old_r = std::make_shared<RecVec>();
    old_r->swap(final_recs);
    defer([old_s, old_r] {
        old_s->reset();
        RecVec().swap(*old_r);
    });
}

void postprocess(Job &job) {
    job.assign_units();
    std::vector<std::vector<int32_t>> units((size_t)job.nunits);
    for (size_t c = 0; c < job.contigs.size(); ++c) units[(size_t)job.contigs[c].unit].push_back((int32_t)c);
    if (job.hits.size() < job.contigs.size()) job.hits.resize(job.contigs.size());
    std::vector<UnitRes> res((size_t)job.nunits);
    std::vector<double> ms((size_t)job.nunits * 4, 0.0);
    const int T = host_threads(job.params);
    // many small units: one thread per unit; few large units: all threads inside each
    int64_t busy = 0;
    for (size_t c = 0; c < job.hits.size(); ++c)
        busy += (job.hits[c].empty() && (c >= job.shits.size() || job.shits[c].empty())) ? 0 : 1;
    // a few units and threads to spare: G groups of T / G threads, each its own
    // pool, take units longest first (a unit's parallel regions carry serial
    // parts and joins that one 16-thread region per unit paid unit by unit)
    const int kGroupThreads = (int)std::max<int64_t>(1, knob(KN_UNIT_GROUP_THREADS));
    const int G = (int)std::min<int64_t>(busy, T / kGroupThreads);
    if (busy >= T) {
        parallel_items(job.nunits, T, [&](int64_t k, int) {
            process_unit(job, units[(size_t)k], job.hits, job.shits, res[(size_t)k], &ms[(size_t)k * 4], 1);
        });
    } else if (G >= 2 && job.nunits >= 2) {
        static std::vector<std::unique_ptr<Pool>> groups;   // persistent, like the global pool
        while ((int)groups.size() < G) groups.push_back(std::make_unique<Pool>());
        std::vector<int32_t> order((size_t)job.nunits);
        std::vector<int64_t> work((size_t)job.nunits, 0);
        for (int32_t k = 0; k < job.nunits; ++k) {
            order[(size_t)k] = k;
            for (int32_t ci : units[(size_t)k]) {
                const size_t c = (size_t)ci;
                work[(size_t)k] += (c < job.hits.size() ? (int64_t)job.hits[c].size() : 0) +
                                   (c < job.shits.size() ? (int64_t)job.shits[c].size() : 0);
            }
        }
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return work[(size_t)a] > work[(size_t)b]; });
        std::atomic<int64_t> next{0};
        const int per = T / G;
        parallel_items(G, G, [&](int64_t g, int) {
            Pool *const prev = Pool::tl_pool;
            Pool::tl_pool = groups[(size_t)g].get();
            try {
                for (;;) {
                    const int64_t q = next.fetch_add(1, std::memory_order_relaxed);
                    if (q >= job.nunits) break;
                    const size_t k = (size_t)order[(size_t)q];
                    process_unit(job, units[k], job.hits, job.shits, res[k], &ms[k * 4], per);
                }
            } catch (...) {
                Pool::tl_pool = prev;
                throw;
            }
            Pool::tl_pool = prev;
        });
    } else {
        for (int32_t k = 0; k < job.nunits; ++k) {
            auto a = std::chrono::steady_clock::now();
            process_unit(job, units[(size_t)k], job.hits, job.shits, res[(size_t)k], &ms[(size_t)k * 4], T);
            if (stats_on())
                std::fprintf(stderr, "  unit %d: %.1f ms total\n", k,
                             std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count());
        }
    }
    // The units with records are kept as they are when each is one contig;
    // otherwise (a unit whose rows interleave several chromosomes) the records
    // are built now.
    job.drop_results();
    auto set = std::make_shared<SurvivorSet>();
    set->job = &job;
    bool one_contig_units = true;
    for (int32_t k = 0; k < job.nunits; ++k) {
        UnitRes &R = res[(size_t)k];
        if (R.items.empty()) continue;
        R.unit = k;
        one_contig_units = one_contig_units && R.contigs == 1;
        set->total += R.items.size();
        set->us.push_back(std::move(R));
    }
    {   // what is left of the units (empty arenas) is released behind the next stage
        auto old = std::make_shared<std::vector<UnitRes>>(std::move(res));
        defer([old] { old->clear(); });
    }
    double built_ms = 0;
    if (one_contig_units) {
        job.keep_survivors(set);
    } else {
        const auto b0 = std::chrono::steady_clock::now();
        set->materialize(job.final_recs, T);
        built_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - b0).count();
        defer([set]() mutable { set.reset(); });
    }
    for (int s = 0; s < 4; ++s) {
        job.stage_ms[2 + s] = 0;
        for (int32_t k = 0; k < job.nunits; ++k) job.stage_ms[2 + s] += ms[(size_t)k * 4 + s];
    }
    job.stage_ms[5] = built_ms;   // records built inside this call (none when the survivors are kept)
    if (stats_on(2))
        std::fprintf(stderr, "[bwtmi] recomputes=%lld (%.1f ms thread-summed; %lld reused walks) merges=%lld canons=%lld "
                     "final=%zu\n", (long long)g_recomputes.exchange(0), g_recompute_ns.exchange(0) / 1e6,
                     (long long)g_walk_reuse.exchange(0), (long long)g_merges.exchange(0),
                     (long long)g_canons.exchange(0), job.count());
    if (stats_on(2))
        std::fprintf(stderr, "[bwtmi] merge tests past the gap test=%lld, same canonical=%lld\n",
                     (long long)g_tests.exchange(0), (long long)g_same.exchange(0));
    if (stats_on(2))
        std::fprintf(stderr, "[bwtmi] fold steps with a fresh current record=%lld (merged %lld), with a merged one=%lld (merged %lld)\n",
                     (long long)g_fresh_tests.exchange(0), (long long)g_fresh_merges.exchange(0),
                     (long long)g_chain_tests.exchange(0), (long long)g_chain_merges.exchange(0));
    if (stats_on(2))
        for (int a = 0; a < 8; ++a)
            for (int b = 0; b < 8; ++b)
                if (int64_t c = g_hist_n[a][b].exchange(0))
                    std::fprintf(stderr, "  m~4^%d len~4^%d: n=%lld %.1f ms (%.2f us)\n", a, b, (long long)c,
                                 g_hist_ns[a][b].load() / 1e6, g_hist_ns[a][b].exchange(0) / 1e3 / (double)c);
    job.postprocessed = true;
}

}  // namespace bwtmi
