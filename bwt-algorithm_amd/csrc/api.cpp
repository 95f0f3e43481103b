// api.cpp -- the extern "C" boundary of libbwtmi.so (include/bwtmi.h): the
// entry points, the job's and the context's device bookkeeping, the lane runner.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cctype>
#include <cstring>
#include <exception>

#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "device.h"
#include "outfile.h"

namespace bwtmi {

static thread_local std::string g_err;

void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}

void fail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    throw Error{code, buf};
}

template <class F>
static int guard(F &&f) {
    try {
        f();
        return BWTMI_OK;
    } catch (const Error &e) {
        g_err = e.msg;
        return e.code;
    } catch (const std::bad_alloc &) {
        g_err = "out of host memory";
        return BWTMI_E_NOMEM;
    } catch (const std::exception &e) {
        g_err = e.what();
        return BWTMI_E_STATE;
    }
}

// device copy of one contig's trimmed sequence, padded for vector loads
struct DevContig {
    DBuf buf;
    int64_t n = -1;
    uint64_t gen = 0;   // Contig::gen of the uploaded content
};

// Host blocks of contig bases (mem.h cached blocks) are registered for DMA the
// first time they are uploaded and stay registered while the block lives
// (cached blocks keep it); the unmap hook drops the registration.
std::mutex g_reg_mu;
std::unordered_map<void *, size_t> g_registered;

void unregister_block(void *p, size_t) {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    auto it = g_registered.find(p);
    if (it == g_registered.end()) return;
    (void)hipHostUnregister(p);
    g_registered.erase(it);
}

// true when [p, p+n) lies in a registered (pinned) block
bool ensure_pinned(const void *base, const void *p, size_t n) {
    const size_t sz = big_block_size(base);
    if (!sz || (const char *)p + n > (const char *)base + sz) return false;
    static std::once_flag hook;
    std::call_once(hook, [] { big_set_unmap_hook(unregister_block); });
    std::lock_guard<std::mutex> lk(g_reg_mu);
    if (g_registered.count(const_cast<void *>(base))) return true;
    if (hipHostRegister(const_cast<void *>(base), sz, hipHostRegisterDefault) != hipSuccess) {
        (void)hipGetLastError();
        return false;   // pageable copy
    }
    g_registered.emplace(const_cast<void *>(base), sz);
    return true;
}

struct JobDev {
    int device = -1;
    std::vector<DevContig> seqs;
    Ctx *bg_ctx = nullptr;   // context whose background work reads these buffers (cleared by its join)
    // the copies now belong on `dev`: another device's are dropped, one entry per contig
    void rebind(int dev, size_t ncontigs) {
        if (device >= 0 && device != dev) {
            for (auto &s : seqs) s.buf.release();
            seqs.clear();
        }
        device = dev;
        seqs.resize(ncontigs);
    }
};

// every entry point that touches a context: join its background work, select the device
static Ctx &use(Ctx &c) {
    ctx_wait(c);
    c.activate();
    return c;
}

// the stream and the two timing events of a new context (the device is current)
static void ctx_create_streams(Ctx &c) {
    HIPCHECK(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
    HIPCHECK(hipEventCreate(&c.ev0));
    HIPCHECK(hipEventCreate(&c.ev1));
}

// v's elements in a malloc block for the caller (bwtmi_free); never null
template <class T, class A>
static T *malloc_copy(const std::vector<T, A> &v) {
    auto *out = (T *)std::malloc(std::max<size_t>(1, v.size()) * sizeof(T));
    if (!out) fail(BWTMI_E_NOMEM, "malloc");
    if (!v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(T));
    return out;
}

}  // namespace bwtmi

using namespace bwtmi;

struct bwtmi_ctx {
    Ctx c;
    DBuf prim[4];   // the caller's arrays of bwtmi_radix_sort / bwtmi_exclusive_scan (no slot of c: the primitives own those)
};
struct bwtmi_index {
    DeviceIndex *d = nullptr;
    bwtmi_ctx *ctx = nullptr;
};
struct bwtmi_job {
    Job j;
    JobDev dev;
    std::unique_ptr<FileWrite> wr;   // a file still being written (bwtmi_job_write_async)
    std::thread units_wr;            // rendered units still being written (bwtmi_job_write_units_async)
    std::exception_ptr units_err;
};

namespace {
// an entry point that touches a job's device buffers through context c: the
// other context whose background work still reads them is joined too
Ctx &job_use(Ctx &c, bwtmi_job *job) {
    if (job->dev.bg_ctx && job->dev.bg_ctx != &c) ctx_wait(*job->dev.bg_ctx);
    return use(c);
}
// the job's file write in flight, if any: wait for it and report its error
void write_join(bwtmi_job *job) {
    if (job->units_wr.joinable()) job->units_wr.join();
    if (job->units_err) {
        std::exception_ptr e = job->units_err;
        job->units_err = nullptr;
        std::rethrow_exception(e);
    }
    if (!job->wr) return;
    std::unique_ptr<FileWrite> w = std::move(job->wr);
    if (!w->finish()) fail(BWTMI_E_IO, "short write to %s", w->path.c_str());
}
// format the job's rows into `path`, the writer thread writing behind the
// formatting; returns with the writer still running (job->wr)
void write_start(bwtmi_job *job, int fmt, const char *path) {
    pool_spin_for_job(job->j);
    job->j.text_join();
    auto w = std::make_unique<FileWrite>(path);
    FileWrite *f = w.get();
    f->th = std::thread([f] { f->run(); });
    const std::function<void(size_t)> on_part = [f](size_t k) { f->part_done(k); };
    render_rows(job->j, fmt, nullptr, f->R, &on_part);   // (throws: ~FileWrite stops the writer, cuts the file)
    f->render_done();
    job->wr = std::move(w);
}
// A caller's array of n elements of `es` bytes on the device (bwtmi_radix_sort,
// bwtmi_exclusive_scan): it starts kPrimPad + skew elements into an allocation
// of n + 3 * kPrimPad elements filled with kPrimFill, so skew = 0 is 16-byte
// aligned, another skew is not (for some element sizes), and the elements on
// both sides are guards that a primitive writing outside [0, n) changes.
constexpr int kPrimPad = 16;
constexpr int kPrimFill = 0xA5;
struct PrimArr {
    DBuf &buf;
    size_t es;
    int64_t n;
    int skew;
    std::vector<uint8_t> img;   // the whole allocation, downloaded
    size_t total() const { return (size_t)(n + 3 * kPrimPad) * es; }
    size_t first() const { return (size_t)(kPrimPad + skew) * es; }
    size_t bytes() const { return (size_t)n * es; }
    template <class T> T *dev() const { return reinterpret_cast<T *>(buf.as<uint8_t>() + first()); }
    void upload(Ctx &c, const void *src) {
        buf.ensure(total());
        HIPCHECK(hipMemsetAsync(buf.p, kPrimFill, total(), c.stream));
        if (src && n) HIPCHECK(hipMemcpyAsync(dev<uint8_t>(), src, bytes(), hipMemcpyHostToDevice, c.stream));
    }
    void download(Ctx &c) {
        img.resize(total());
        HIPCHECK(hipMemcpyAsync(img.data(), buf.p, total(), hipMemcpyDeviceToHost, c.stream));
    }
    const uint8_t *data() const { return img.data() + first(); }
    // after download and a stream wait: the guards still hold the fill
    void check_guards(const char *what) const {
        for (size_t i = 0; i < img.size(); i = i + 1 == first() ? first() + bytes() : i + 1)
            if (img[i] != kPrimFill)
                fail(BWTMI_E_STATE, "%s: byte %lld outside the array's %lld bytes was written", what,
                     (long long)i - (long long)first(), (long long)bytes());
    }
    void check_same(const void *src, const char *what) const {
        if (n && std::memcmp(data(), src, bytes()) != 0) fail(BWTMI_E_STATE, "%s: the input array changed", what);
    }
};
}  // namespace

// readers of contig bytes join a deferred host pass first (bwtmi_job_load_fasta_dev)
#define TEXT_JOIN(job) const_cast<bwtmi_job *>(job)->j.text_join()

#define CHECK_ARG(cond, msg)                     \
    do {                                         \
        if (!(cond)) fail(BWTMI_E_ARG, "%s", msg); \
    } while (0)

extern "C" {

const char *bwtmi_last_error(void) { return g_err.c_str(); }
// sha256 of the sources the library was built from (csrc/*.cpp *.h *.hip and
// include/bwtmi.h in path order; generated by the Makefile into build/srchash.c)
extern "C" const char bwtmi_src_sha256[];
const char *bwtmi_source_hash(void) { return bwtmi_src_sha256; }
const char *bwtmi_version(void) {
    static const std::string v = std::string("bwtmi 0.5 (gfx950) src ") + bwtmi_src_sha256;
    return v.c_str();
}
void bwtmi_free(void *p) { std::free(p); }

int bwtmi_device_count(int *count) {
    return guard([&] {
        CHECK_ARG(count, "null count");
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        *count = (e == hipSuccess) ? n : 0;
    });
}

// Host threads next to the GPU: a process free to run on both sockets of a
// box spread its 16 threads (and their first-touch pages) over both, and the
// W = 8 shard step came out at 8.0 or 9.0 ms from run to run; pinned to either
// node every run took 7.5-8.3 ms (r04x/r04y).  Local rank r drives device
// r mod (visible devices) -- LOCAL_RANK / LOCAL_WORLD_SIZE of the launcher --
// so the ranks sharing this GPU's node are counted from their own GPUs.
static bool bind_host_for(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return false;
    }
    const char *lw_e = std::getenv("LOCAL_WORLD_SIZE");
    const char *lr_e = std::getenv("LOCAL_RANK");
    const int lw = std::max(1, lw_e ? std::atoi(lw_e) : 1);
    int lr = lr_e ? std::atoi(lr_e) : device;
    if (lr < 0 || lr >= lw) lr = 0;
    std::vector<std::string> pci((size_t)lw);
    for (int r = 0; r < lw; ++r) {
        const int d = r == lr ? device : r % ndev;
        char bus[64] = {0};
        if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, d) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        pci[(size_t)r] = bus;
    }
    return bind_host_numa(lr, pci);
}

int bwtmi_open(int device, bwtmi_ctx **out) {
    return guard([&] {
        CHECK_ARG(out, "null out");
        *out = nullptr;
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
            fail(BWTMI_E_NODEVICE, "no HIP device available (libbwtmi has no CPU fallback)");
        if (device < 0 || device >= n) fail(BWTMI_E_NODEVICE, "device %d out of range (%d devices)", device, n);
        hipDeviceProp_t prop;
        HIPCHECK(hipGetDeviceProperties(&prop, device));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            fail(BWTMI_E_NODEVICE, "device %d is %s; libbwtmi is built for gfx950 only", device, prop.gcnArchName);
        auto *ctx = new bwtmi_ctx();
        ctx->c.device = device;
        HIPCHECK(hipSetDevice(device));
        // host threads next to the GPU only when asked for (bwtmi_bind_host, or
        // BWTMI_NUMA_BIND=1 here): a library call never changes the caller's
        // affinity on its own
        if (knob(KN_NUMA_BIND)) bind_host_for(device);
        // how a host thread waits for the device: the background index build
        // waits on the device while every host thread post-processes, so a
        // spinning wait would take a core from them -- blocking waits (r02az, C3:
        // 1949 vs 1895 Mbp/s over 3 runs each); the scan's short waits poll
        // (scan_wait)
        if (hipSetDeviceFlags(hipDeviceScheduleBlockingSync) != hipSuccess) (void)hipGetLastError();
        ctx_create_streams(ctx->c);
        *out = ctx;
    });
}

static void ctx_release(Ctx &c) {
    (void)hipStreamSynchronize(c.stream);
    for (auto &l : c.lanes) ctx_release(*l);
    c.lanes.clear();
    if (c.scratch_index) index_free(c.scratch_index);
    c.scratch_index = nullptr;
    for (auto &s : c.slot) s.release();
    c.chk.release();
    c.lb_ticket.release();
    for (auto &h : c.host) h.release();
    c.mbox.release();
    for (hipEvent_t e : c.evpool) (void)hipEventDestroy(e);
    c.evpool.clear();
    (void)hipEventDestroy(c.ev0);
    (void)hipEventDestroy(c.ev1);
    (void)hipStreamDestroy(c.stream);
}

// lane k of c (k >= 1): a context of its own on c's device, created on first use
static Ctx &scan_lane(Ctx &c, size_t k) {
    while (c.lanes.size() < k) {
        auto l = std::make_unique<Ctx>();
        l->device = c.device;
        ctx_create_streams(*l);
        c.lanes.push_back(std::move(l));
    }
    Ctx &l = *c.lanes[k - 1];
    l.ktiming = c.ktiming;
    l.kfilter = c.kfilter;
    l.timing = c.timing;
    return l;
}

int bwtmi_bind_host(bwtmi_ctx *ctx, int on, int *changed) {
    return guard([&] {
        CHECK_ARG(ctx, "null argument");
        const bool b = on ? bind_host_for(ctx->c.device) : unbind_host();
        if (changed) *changed = b ? 1 : 0;
    });
}

int bwtmi_host_binding_plan(const char *sysroot, int local_rank, const char *rank_pci, int threads, int smt,
                            const char *allowed, char *out, int64_t cap, int *node, int *ranks_on_node) {
    return guard([&] {
        CHECK_ARG(sysroot && rank_pci && allowed && out && cap > 0, "null argument");
        std::vector<std::string> pci;
        for (const char *p = rank_pci; *p;) {
            const char *e = std::strchr(p, ',');
            pci.emplace_back(p, e ? (size_t)(e - p) : std::strlen(p));
            p = e ? e + 1 : p + std::strlen(p);
        }
        cpu_set_t al, cs;
        if (!parse_cpulist(allowed, al)) fail(BWTMI_E_ARG, "bad cpulist '%s'", allowed);
        int nd = -1, peers = 0;
        const bool b = plan_host_binding(sysroot, local_rank, pci, threads, smt != 0, al, cs, &nd, &peers);
        const std::string str = b ? cpulist_str(cs) : std::string();
        if ((int64_t)str.size() + 1 > cap) fail(BWTMI_E_ARG, "output buffer too small");
        std::memcpy(out, str.c_str(), str.size() + 1);
        if (node) *node = nd;
        if (ranks_on_node) *ranks_on_node = peers;
    });
}

int bwtmi_close(bwtmi_ctx *ctx) {
    return guard([&] {
        if (!ctx) return;
        ctx_join(ctx->c);   // a background error dies with the context
        ctx->c.activate();
        ctx_release(ctx->c);
        for (auto &b : ctx->prim) b.release();
        delete ctx;
    });
}

int bwtmi_last_timing(bwtmi_ctx *ctx, double *out3) {
    return guard([&] {
        CHECK_ARG(ctx && out3, "null argument");
        ctx_wait(ctx->c);
        out3[0] = ctx->c.last_total_ms;
        out3[1] = ctx->c.last_dom_ms;
        out3[2] = ctx->c.last_dom_launches;
    });
}

int bwtmi_kernel_stats_filter(bwtmi_ctx *ctx, const char *name) {
    return guard([&] {
        CHECK_ARG(ctx, "null ctx");
        ctx_wait(ctx->c);
        ctx->c.kfilter = name ? name : "";
    });
}

int bwtmi_kernel_stats(bwtmi_ctx *ctx, int enable, int reset, char *out, int64_t cap) {
    return guard([&] {
        CHECK_ARG(ctx, "null ctx");
        Ctx &c = ctx->c;
        ctx_wait(c);
        if (!c.pending.empty()) {   // launches of calls that end without resolving their timers
            HIPCHECK(hipStreamSynchronize(c.stream));
            c.kresolve();
        }
        std::string s;
        char line[160];
        for (auto &k : c.kstats) {
            snprintf(line, sizeof line, "%s %.6f %lld %.0f\n", k.first.c_str(), k.second.ms,
                     (long long)k.second.launches, k.second.bytes);
            s += line;
        }
        if (out && cap > 0) {
            const size_t m = std::min<size_t>((size_t)cap - 1, s.size());
            std::memcpy(out, s.data(), m);
            out[m] = 0;
        }
        if (reset) c.kstats.clear();
        c.ktiming = enable != 0;
    });
}

// ------------------------------------------------------------ strict scan
static void upload_text(Ctx &c, DBuf &buf, const uint8_t *seq, int64_t n) {
    buf.ensure((size_t)n + 128);
    HIPCHECK(hipMemsetAsync((uint8_t *)buf.p + n, 0, 128, c.stream));
    if (n) HIPCHECK(hipMemcpyAsync(buf.p, seq, (size_t)n, hipMemcpyHostToDevice, c.stream));
}

int bwtmi_strict_scan(bwtmi_ctx *ctx, const uint8_t *seq, int64_t n, int32_t min_unit, int32_t max_unit,
                      int32_t max_mismatch, int32_t min_copies, bwtmi_hit **hits, int64_t *nhits) {
    return guard([&] {
        CHECK_ARG(ctx && hits && nhits && (seq || n == 0) && n >= 0, "bad argument");
        CHECK_ARG(max_mismatch >= 0, "max_mismatch must be >= 0");
        *hits = nullptr;
        *nhits = 0;
        if (n > 0 && seq[n - 1] == '$') --n;   // bwt.py:1915-1916
        Ctx &c = ctx->c;
        use(c);
        upload_text(c, c.slot[S_TEXT], seq, n);
        ScanResult r;
        if (max_mismatch > 0)   // Hamming-tolerant adjacency (library calls)
            strict_scan_mm_device(c, c.slot[S_TEXT].as<uint8_t>(), n, min_unit, max_unit, max_mismatch, min_copies,
                                  r.hits);
        else
            strict_scan_device(c, c.slot[S_TEXT].as<uint8_t>(), n, min_unit, max_unit, min_copies, r);
        *nhits = (int64_t)r.hits.size();
        *hits = malloc_copy(r.hits);
    });
}

// the device screen on a caller's hit list (tests, embedders): the hits go to
// the slot the scan leaves its own in, screen_hits_device runs as it does there
int bwtmi_screen_hits(bwtmi_ctx *ctx, const bwtmi_hit *hits, int64_t n, int64_t text_len, int32_t min_copies,
                      int32_t drop, int64_t maxlen, int64_t **out, int64_t *nout) {
    return guard([&] {
        CHECK_ARG(ctx && out && nout && (hits || n == 0) && n >= 0, "bad argument");
        *out = nullptr;
        *nout = 0;
        CHECK_ARG(text_len >= 0 && min_copies >= 1 && maxlen >= -1, "bad argument");
        // the level kernels index a bucket table by end >> 6: no span past text_len reaches them
        int64_t longest = 0;
        int32_t lmax = 1;
        for (int64_t i = 0; i < n; ++i) {
            const bwtmi_hit &h = hits[i];
            if (h.start < 0 || h.end <= h.start || h.end > text_len || h.prim_len < 1)
                fail(BWTMI_E_ARG, "hit %lld [%lld, %lld) prim %d outside 0 <= start < end <= %lld, prim >= 1",
                     (long long)i, (long long)h.start, (long long)h.end, (int)h.prim_len, (long long)text_len);
            longest = std::max(longest, h.end - h.start);
            lmax = std::max(lmax, h.prim_len);
        }
        CHECK_ARG(maxlen < 0 || maxlen >= longest, "maxlen is below the longest span");
        std::vector<int64_t> rows;
        if (n > 0) {
            Ctx &c = ctx->c;
            use(c);
            c.slot[S_HITS].ensure((size_t)n * sizeof(bwtmi_hit));
            HIPCHECK(hipMemcpyAsync(c.slot[S_HITS].p, hits, (size_t)n * sizeof(bwtmi_hit), hipMemcpyHostToDevice,
                                    c.stream));
            ScreenedVec sv;
            screen_hits_device(c, c.slot[S_HITS].as<bwtmi_hit>(), n, text_len, lmax, sv, maxlen, min_copies, drop != 0);
            const int64_t nk = sv.size();
            sv.wait(nk);
            c.kresolve();
            rows.resize((size_t)nk * 4);
            for (int64_t k = 0; k < nk; ++k) {
                int64_t s, len, prim;
                const bool cut = sv.get(k, s, len, prim);
                int64_t *r = rows.data() + 4 * k;
                r[0] = s;
                r[1] = len;
                r[2] = prim;
                r[3] = cut ? 1 : 0;
            }
        }
        *nout = (int64_t)rows.size() / 4;
        *out = malloc_copy(rows);
    });
}

// ------------------------------------------------------------ primitives
// the radix sorts of radix.hip on a caller's arrays (tests, embedders): the
// arrays go to buffers of the entry's own, the primitive runs as its callers
// run it, the results come back into the caller's arrays
int bwtmi_radix_sort(bwtmi_ctx *ctx, int32_t kind, void *keys, void *vals, int64_t n, int32_t bit0, int32_t bit1,
                     int32_t skew) {
    return guard([&] {
        CHECK_ARG(ctx, "null context");
        CHECK_ARG(kind >= BWTMI_SORT_K64V64 && kind <= BWTMI_SORT_PASS_K32, "unknown sort kind");
        const size_t kb = kind <= BWTMI_SORT_K64 ? 8 : kind == BWTMI_SORT_K16V32 ? 2 : 4;
        const size_t vb = kind == BWTMI_SORT_K64V64 ? 8 : kind == BWTMI_SORT_K64 ? 0 : 4;
        CHECK_ARG(n >= 0 && n < (int64_t{1} << 32), "n outside 0 .. 2^32 - 1");
        CHECK_ARG(n == 0 || (keys && (vals || !vb)), "null array");
        CHECK_ARG(bit0 >= 0 && bit1 <= (int32_t)(8 * kb) && bit0 < bit1 && (bit1 - bit0) % 8 == 0,
                  "need 0 <= bit0 < bit1 <= the key width and a whole number of 8-bit digits");
        CHECK_ARG(kind != BWTMI_SORT_PASS_K32 || bit1 == bit0 + 8, "one pass sorts one digit: bit1 = bit0 + 8");
        CHECK_ARG(skew >= 0 && skew < kPrimPad, "skew outside 0..15");
        if (n == 0) return;
        Ctx &c = ctx->c;
        use(c);
        PrimArr k{ctx->prim[0], kb, n, skew}, v{ctx->prim[1], vb, vb ? n : 0, skew};
        k.upload(c, keys);
        if (vb) v.upload(c, vals);
        if (kind == BWTMI_SORT_PASS_K32) {
            PrimArr ko{ctx->prim[2], kb, n, skew}, vo{ctx->prim[3], vb, n, skew};
            ko.upload(c, nullptr);
            vo.upload(c, nullptr);
            radix_pass_k32(c, k.dev<uint32_t>(), v.dev<uint32_t>(), ko.dev<uint32_t>(), vo.dev<uint32_t>(), n, bit0);
            for (PrimArr *a : {&k, &v, &ko, &vo}) a->download(c);
            HIPCHECK(hipStreamSynchronize(c.stream));
            c.kresolve();
            c.checks_verify("bwtmi_radix_sort");
            for (PrimArr *a : {&k, &v, &ko, &vo}) a->check_guards("bwtmi_radix_sort");
            k.check_same(keys, "bwtmi_radix_sort (pass keys)");
            v.check_same(vals, "bwtmi_radix_sort (pass values)");
            std::memcpy(keys, ko.data(), ko.bytes());
            std::memcpy(vals, vo.data(), vo.bytes());
            return;
        }
        switch (kind) {
        case BWTMI_SORT_K64V64: radix_sort_pairs(c, k.dev<uint64_t>(), v.dev<uint64_t>(), n, bit0, bit1); break;
        case BWTMI_SORT_K64V32: radix_sort_pairs32(c, k.dev<uint64_t>(), v.dev<uint32_t>(), n, bit0, bit1); break;
        case BWTMI_SORT_K64: radix_sort_pairs32(c, k.dev<uint64_t>(), nullptr, n, bit0, bit1); break;
        case BWTMI_SORT_K32V32: radix_sort_pairs_k32(c, k.dev<uint32_t>(), v.dev<uint32_t>(), n, bit0, bit1); break;
        default: radix_sort_pairs_k16(c, k.dev<uint16_t>(), v.dev<uint32_t>(), n, bit0, bit1); break;
        }
        k.download(c);
        if (vb) v.download(c);
        HIPCHECK(hipStreamSynchronize(c.stream));
        c.kresolve();
        c.checks_verify("bwtmi_radix_sort");
        k.check_guards("bwtmi_radix_sort");
        if (vb) v.check_guards("bwtmi_radix_sort");
        std::memcpy(keys, k.data(), k.bytes());
        if (vb) std::memcpy(vals, v.data(), v.bytes());
    });
}

// the exclusive scans of radix.hip on a caller's array(s)
int bwtmi_exclusive_scan(bwtmi_ctx *ctx, int32_t kind, const void *in, void *out, int64_t n, int32_t rows,
                         int64_t stride, int32_t skew, int32_t in_place, int64_t epoch) {
    return guard([&] {
        CHECK_ARG(ctx, "null context");
        CHECK_ARG(kind == BWTMI_SCAN_U32 || kind == BWTMI_SCAN_I64, "unknown scan kind");
        CHECK_ARG(n >= 0 && n < (int64_t{1} << 32) && rows >= 1 && rows <= 65536 && stride >= 0 &&
                      stride < (int64_t{1} << 32), "n, rows or stride out of range");
        CHECK_ARG(kind == BWTMI_SCAN_U32 || rows == 1, "the 64-bit scan takes one row");
        CHECK_ARG(rows == 1 || stride >= n, "rows overlap: stride < n");
        CHECK_ARG(n == 0 || (in && out), "null array");
        CHECK_ARG(skew >= 0 && skew < kPrimPad, "skew outside 0..15");
        Ctx &c = ctx->c;
        use(c);   // (joins background work that draws epochs)
        // the epoch only ever moves forward: a granule of a later epoch than the
        // next launch's cannot exist, so no stale granule can match
        CHECK_ARG(epoch == 0 || (epoch > (int64_t)c.lb_epoch && epoch < (int64_t{1} << 30)),
                  "epoch must be above the context's and below 2^30");
        if (n == 0) return;
        if (epoch) c.lb_epoch = (uint32_t)epoch;
        const size_t es = kind == BWTMI_SCAN_U32 ? 4 : 8;
        const int64_t total = (int64_t)(rows - 1) * stride + n;
        PrimArr a{ctx->prim[0], es, total, skew}, b{ctx->prim[1], es, total, skew};
        a.upload(c, in);
        if (!in_place) b.upload(c, out);   // what the scan does not write stays the caller's
        PrimArr &o = in_place ? a : b;
        if (kind == BWTMI_SCAN_I64) exclusive_scan<int64_t>(c, a.dev<int64_t>(), o.dev<int64_t>(), n);
        else if (rows == 1) exclusive_scan<uint32_t>(c, a.dev<uint32_t>(), o.dev<uint32_t>(), n);
        else exclusive_scan_rows(c, a.dev<uint32_t>(), o.dev<uint32_t>(), n, rows, stride);
        a.download(c);
        if (!in_place) b.download(c);
        HIPCHECK(hipStreamSynchronize(c.stream));
        c.kresolve();
        a.check_guards("bwtmi_exclusive_scan");
        if (!in_place) {
            b.check_guards("bwtmi_exclusive_scan");
            a.check_same(in, "bwtmi_exclusive_scan");
        }
        std::memcpy(out, o.data(), o.bytes());
    });
}

// ------------------------------------------------------------ index
int bwtmi_index_build(bwtmi_ctx *ctx, const uint8_t *text, int64_t n, int32_t sa_sample, int32_t occ_sample,
                      uint32_t flags, bwtmi_index **out) {
    return guard([&] {
        BWTMI_STAGE("bwtmi:index");
        CHECK_ARG(ctx && out && (text || n == 0) && n >= 0 && sa_sample > 0 && occ_sample > 0, "bad argument");
        *out = nullptr;
        Ctx &c = ctx->c;
        use(c);
        upload_text(c, c.slot[S_TEXT], text, n);
        auto *idx = new bwtmi_index();
        idx->ctx = ctx;
        try {
            idx->d = index_build_device(c, c.slot[S_TEXT].as<uint8_t>(), n, sa_sample, occ_sample, flags);
        } catch (...) {
            delete idx;
            throw;
        }
        *out = idx;
    });
}

int bwtmi_index_free(bwtmi_index *idx) {
    return guard([&] {
        if (!idx) return;
        use(idx->ctx->c);
        index_free(idx->d);
        delete idx;
    });
}

int64_t bwtmi_index_size(const bwtmi_index *idx) { return idx ? index_n(idx->d) : -1; }
int bwtmi_index_has_reverse(const bwtmi_index *idx) { return idx && index_has_reverse(idx->d) ? 1 : 0; }
int64_t bwtmi_index_occ_len(const bwtmi_index *idx) { return idx ? index_occ_len(idx->d) : -1; }
int64_t bwtmi_index_sampled_len(const bwtmi_index *idx) { return idx ? index_sampled_len(idx->d) : -1; }
int64_t bwtmi_index_kmer_count(const bwtmi_index *idx) { return idx ? index_kmer_count(idx->d) : -1; }

int bwtmi_index_get_sa(const bwtmi_index *idx, int32_t *sa) {
    return guard([&] { CHECK_ARG(idx && sa, "null"); index_get_sa(use(idx->ctx->c), idx->d, sa); });
}
int bwtmi_index_get_bwt(const bwtmi_index *idx, uint8_t *bwt) {
    return guard([&] { CHECK_ARG(idx && bwt, "null"); index_get_bwt(use(idx->ctx->c), idx->d, bwt); });
}
int bwtmi_index_get_counts(const bwtmi_index *idx, int64_t *totals, int64_t *C) {
    return guard([&] { CHECK_ARG(idx && totals && C, "null"); index_get_counts(idx->d, totals, C); });
}
int bwtmi_index_get_occ(const bwtmi_index *idx, uint8_t code, int32_t *cp) {
    return guard([&] { CHECK_ARG(idx && cp, "null"); index_get_occ(use(idx->ctx->c), idx->d, code, cp); });
}
int bwtmi_index_get_sampled(const bwtmi_index *idx, int32_t *vals) {
    return guard([&] { CHECK_ARG(idx && vals, "null"); index_get_sampled(use(idx->ctx->c), idx->d, vals); });
}
int bwtmi_index_get_kmer(const bwtmi_index *idx, int64_t *offsets, int32_t *positions) {
    return guard([&] {
        CHECK_ARG(idx && offsets && positions, "null");
        index_get_kmer(use(idx->ctx->c), idx->d, offsets, positions);
    });
}
int bwtmi_index_lcp(bwtmi_ctx *ctx, bwtmi_index *idx, int32_t *lcp) {
    return guard([&] {
        CHECK_ARG(ctx && idx && lcp, "null");
        use(ctx->c);
        index_lcp(ctx->c, idx->d, lcp);
    });
}
int bwtmi_backward_search_batch(bwtmi_ctx *ctx, bwtmi_index *idx, const uint8_t *pats, const int64_t *off,
                                int64_t npat, int64_t *sp_ep) {
    return guard([&] {
        CHECK_ARG(ctx && idx && off && sp_ep && npat >= 0, "bad argument");
        use(ctx->c);
        index_backward_search(ctx->c, idx->d, pats, off, npat, sp_ep);
    });
}

int bwtmi_index_locate_batch(bwtmi_ctx *ctx, bwtmi_index *idx, const uint8_t *pats, const int64_t *off, int64_t npat,
                             int32_t max_mismatch, uint32_t flags, int64_t max_candidates, int64_t **hit_off,
                             int64_t **pos, uint8_t **mm, uint8_t **strand, int64_t *nhits, int64_t *candidates) {
    return guard([&] {
        CHECK_ARG(ctx && idx && off && hit_off && pos && mm && strand && nhits && npat >= 0, "bad argument");
        CHECK_ARG(pats || npat == 0, "null patterns");
        *hit_off = *pos = nullptr;
        *mm = *strand = nullptr;
        *nhits = 0;
        if (candidates) *candidates = 0;
        CHECK_ARG((flags & ~BWTMI_LOCATE_BOTH_STRANDS) == 0, "unknown locate flag");
        use(ctx->c);
        LocateResult r;
        try {
            index_locate_batch(ctx->c, idx->d, pats, off, npat, max_mismatch, (flags & BWTMI_LOCATE_BOTH_STRANDS) != 0,
                               max_candidates, r);
        } catch (...) {
            if (candidates) *candidates = r.candidates;   // the count a tripped cap reports
            throw;
        }
        if (candidates) *candidates = r.candidates;
        *hit_off = malloc_copy(r.hit_off);
        *pos = malloc_copy(r.pos);
        *mm = malloc_copy(r.mm);
        *strand = malloc_copy(r.strand);
        *nhits = (int64_t)r.pos.size();
    });
}

// the two SMEM entries: `search` is index_smem_batch or index_smem_long_batch
using SmemSearch = void (*)(Ctx &, DeviceIndex *, const uint8_t *, const int64_t *, int64_t, int32_t, bool, int64_t,
                            int64_t, SmemResult &);
static int smem_entry(bwtmi_ctx *ctx, bwtmi_index *idx, const uint8_t *qs, const int64_t *off, int64_t nq,
                      int32_t min_len, uint32_t flags, int64_t max_occ, int64_t max_positions, int64_t **smem_off,
                      int32_t **qstart, int32_t **qend, uint8_t **strand, int64_t **count, int64_t **pos_off,
                      int64_t **pos, int64_t *nsmem, int64_t *npos, int64_t *positions_total, int64_t *work,
                      int64_t *steps, SmemSearch search) {
    return guard([&] {
        if (steps) *steps = 0;
        CHECK_ARG(ctx && idx && off && smem_off && qstart && qend && strand && count && pos_off && pos && nsmem && npos &&
                      nq >= 0,
                  "bad argument");
        CHECK_ARG(qs || nq == 0, "null queries");
        *smem_off = *count = *pos_off = *pos = nullptr;
        *qstart = *qend = nullptr;
        *strand = nullptr;
        *nsmem = *npos = 0;
        if (positions_total) *positions_total = 0;
        if (work) *work = 0;
        CHECK_ARG((flags & ~BWTMI_SMEM_BOTH_STRANDS) == 0, "unknown smem flag");
        use(ctx->c);
        SmemResult r;
        try {
            search(ctx->c, idx->d, qs, off, nq, min_len, (flags & BWTMI_SMEM_BOTH_STRANDS) != 0, max_occ, max_positions,
                   r);
        } catch (...) {
            if (positions_total) *positions_total = r.positions_total;   // the count a tripped cap reports
            throw;
        }
        if (positions_total) *positions_total = r.positions_total;
        if (work) *work = r.work;
        if (steps) *steps = r.steps;
        *smem_off = malloc_copy(r.smem_off);
        *qstart = malloc_copy(r.qstart);
        *qend = malloc_copy(r.qend);
        *strand = malloc_copy(r.strand);
        *count = malloc_copy(r.count);
        *pos_off = malloc_copy(r.pos_off);
        *pos = malloc_copy(r.pos);
        *nsmem = (int64_t)r.qstart.size();
        *npos = (int64_t)r.pos.size();
    });
}

int bwtmi_index_smem_batch(bwtmi_ctx *ctx, bwtmi_index *idx, const uint8_t *qs, const int64_t *off, int64_t nq,
                           int32_t min_len, uint32_t flags, int64_t max_occ, int64_t max_positions, int64_t **smem_off,
                           int32_t **qstart, int32_t **qend, uint8_t **strand, int64_t **count, int64_t **pos_off,
                           int64_t **pos, int64_t *nsmem, int64_t *npos, int64_t *positions_total, int64_t *work) {
    return smem_entry(ctx, idx, qs, off, nq, min_len, flags, max_occ, max_positions, smem_off, qstart, qend, strand, count,
                      pos_off, pos, nsmem, npos, positions_total, work, nullptr, index_smem_batch);
}

int bwtmi_index_smem_long_batch(bwtmi_ctx *ctx, bwtmi_index *idx, const uint8_t *qs, const int64_t *off, int64_t nq,
                                int32_t min_len, uint32_t flags, int64_t max_occ, int64_t max_positions,
                                int64_t **smem_off, int32_t **qstart, int32_t **qend, uint8_t **strand,
                                int64_t **count, int64_t **pos_off, int64_t **pos, int64_t *nsmem, int64_t *npos,
                                int64_t *positions_total, int64_t *work, int64_t *steps) {
    return smem_entry(ctx, idx, qs, off, nq, min_len, flags, max_occ, max_positions, smem_off, qstart, qend, strand, count,
                      pos_off, pos, nsmem, npos, positions_total, work, steps, index_smem_long_batch);
}

// ------------------------------------------------------------ chaining
// the caller's parameters with the defaults filled in, checked
static ChainParams chain_params(const bwtmi_chain_params *p) {
    ChainParams r;
    if (!p) return r;
    CHECK_ARG(p->reserved[0] == 0 && p->reserved[1] == 0 && p->reserved[2] == 0, "chain: reserved fields must be 0");
    if (p->max_gap > 0) r.max_gap = p->max_gap;
    if (p->bandwidth > 0) r.bandwidth = p->bandwidth;
    if (p->max_pred > 0) r.max_pred = p->max_pred;
    if (p->min_score > 0) r.min_score = p->min_score;
    if (p->min_anchors > 0) r.min_anchors = p->min_anchors;
    if (r.max_pred > 4096) fail(BWTMI_E_ARG, "chain: max_pred %d is above 4096", (int)r.max_pred);
    if (r.bandwidth > r.max_gap)
        fail(BWTMI_E_ARG, "chain: bandwidth %d is above max_gap %d", (int)r.bandwidth, (int)r.max_gap);
    return r;
}

int bwtmi_chain_anchors(bwtmi_ctx *ctx, const int64_t *group_off, int64_t ng, const int32_t *q, const int64_t *r,
                        const int32_t *len, const bwtmi_chain_params *params, int64_t **chain_off, int32_t **score,
                        int32_t **n_anchors, int32_t **qstart, int32_t **qend, int64_t **rstart, int64_t **rend,
                        int64_t **member_off, int64_t **member, int64_t *nchain, int64_t *nmember, int64_t *evals) {
    return guard([&] {
        CHECK_ARG(ctx && group_off && ng >= 0 && chain_off && score && n_anchors && qstart && qend && rstart && rend &&
                      member_off && member && nchain && nmember,
                  "bad argument");
        const ChainParams p = chain_params(params);
        CHECK_ARG(group_off[0] == 0, "chain: group_off[0] must be 0");
        for (int64_t g = 0; g < ng; ++g)
            if (group_off[g + 1] < group_off[g])
                fail(BWTMI_E_ARG, "chain: group_off decreases at group %lld", (long long)g);
        const int64_t na = group_off[ng];
        CHECK_ARG(na == 0 || (q && r && len), "chain: null anchor array");
        for (int64_t i = 0; i < na; ++i)
            if (len[i] < 1 || q[i] < 0 || r[i] < 0 || (int64_t)q[i] + len[i] > (int64_t{1} << 24) ||
                r[i] + len[i] > (int64_t{1} << 32))
                fail(BWTMI_E_ARG, "chain: anchor %lld (q %d, r %lld, len %d) outside len >= 1, 0 <= q, q + len <= 2^24, "
                     "0 <= r, r + len <= 2^32", (long long)i, (int)q[i], (long long)r[i], (int)len[i]);
        ChainResult res;
        chain_anchors_device(use(ctx->c), group_off, ng, q, r, len, p, res);
        *chain_off = malloc_copy(res.chain_off);
        *score = malloc_copy(res.score);
        *n_anchors = malloc_copy(res.n_anchors);
        *qstart = malloc_copy(res.qstart);
        *qend = malloc_copy(res.qend);
        *rstart = malloc_copy(res.rstart);
        *rend = malloc_copy(res.rend);
        *member_off = malloc_copy(res.member_off);
        *member = malloc_copy(res.member);
        *nchain = (int64_t)res.score.size();
        *nmember = (int64_t)res.member.size();
        if (evals) *evals = res.evals;
    });
}

int bwtmi_index_map_batch(bwtmi_ctx *ctx, bwtmi_index *idx, const uint8_t *qs, const int64_t *off, int64_t nq,
                          int32_t min_len, uint32_t flags, int64_t max_occ, int64_t max_positions,
                          const bwtmi_chain_params *params, int64_t **chain_off, uint8_t **strand, int32_t **score,
                          int32_t **n_anchors, int32_t **qstart, int32_t **qend, int64_t **rstart, int64_t **rend,
                          int64_t **member_off, int32_t **member_q, int64_t **member_r, int32_t **member_len,
                          int64_t *nchain, int64_t *nmember, int64_t *positions_total, int64_t *skipped_smems,
                          int64_t *anchors, int64_t *evals) {
    return guard([&] {
        CHECK_ARG(ctx && idx && off && nq >= 0 && chain_off && strand && score && n_anchors && qstart && qend && rstart &&
                      rend && member_off && member_q && member_r && member_len && nchain && nmember,
                  "bad argument");
        CHECK_ARG(qs || nq == 0, "null queries");
        *chain_off = *rstart = *rend = *member_off = *member_r = nullptr;
        *score = *n_anchors = *qstart = *qend = *member_q = *member_len = nullptr;
        *strand = nullptr;
        *nchain = *nmember = 0;
        for (int64_t *v : {positions_total, skipped_smems, anchors, evals})
            if (v) *v = 0;
        CHECK_ARG((flags & ~(BWTMI_SMEM_BOTH_STRANDS | BWTMI_MAP_LONG)) == 0, "unknown map flag");
        const ChainParams p = chain_params(params);
        Ctx &c = use(ctx->c);
        MapResult r;
        try {
            index_map_batch(c, idx->d, qs, off, nq, min_len, (flags & BWTMI_SMEM_BOTH_STRANDS) != 0,
                            (flags & BWTMI_MAP_LONG) != 0, max_occ, max_positions, p, r);
        } catch (...) {
            if (positions_total) *positions_total = r.positions_total;   // the count a tripped cap reports
            throw;
        }
        if (positions_total) *positions_total = r.positions_total;
        if (skipped_smems) *skipped_smems = r.skipped_smems;
        if (anchors) *anchors = r.anchors;
        if (evals) *evals = r.evals;
        *chain_off = malloc_copy(r.chain_off);
        *strand = malloc_copy(r.strand);
        *score = malloc_copy(r.score);
        *n_anchors = malloc_copy(r.n_anchors);
        *qstart = malloc_copy(r.qstart);
        *qend = malloc_copy(r.qend);
        *rstart = malloc_copy(r.rstart);
        *rend = malloc_copy(r.rend);
        *member_off = malloc_copy(r.member_off);
        *member_q = malloc_copy(r.mq);
        *member_r = malloc_copy(r.mr);
        *member_len = malloc_copy(r.mlen);
        *nchain = (int64_t)r.score.size();
        *nmember = (int64_t)r.mq.size();
    });
}

// ------------------------------------------------------------ selection
int bwtmi_select_chains(bwtmi_ctx *ctx, const int64_t *chain_off, int64_t ng, const int32_t *score,
                        const int32_t *qstart, const int32_t *qend, const bwtmi_select_params *params,
                        int32_t **parent, int32_t **sub, uint8_t **mapq, uint8_t **keep, int64_t *n_primary,
                        int64_t *n_kept) {
    return guard([&] {
        CHECK_ARG(ctx && parent && sub && mapq && keep, "bad argument");
        *parent = *sub = nullptr;
        *mapq = *keep = nullptr;
        if (n_primary) *n_primary = 0;
        if (n_kept) *n_kept = 0;
        SelectParams p;
        if (params) {
            for (int32_t v : params->reserved) CHECK_ARG(v == 0, "select: reserved fields must be 0");
            if (params->mask >= 0) p.mask = params->mask;
            if (params->pri_ratio >= 0) p.pri_ratio = params->pri_ratio;
            if (params->best_n >= 0) p.best_n = params->best_n;
            if (params->full >= 0) p.full = params->full;
        }
        if (p.mask < 1 || p.mask > 100) fail(BWTMI_E_ARG, "select: mask %d outside 1..100", (int)p.mask);
        if (p.pri_ratio > 100) fail(BWTMI_E_ARG, "select: pri_ratio %d outside 0..100", (int)p.pri_ratio);
        if (p.full < 1 || p.full > (1 << 20)) fail(BWTMI_E_ARG, "select: full %d outside 1..2^20", (int)p.full);
        CHECK_ARG(ng >= 0, "select: ng must not be negative");
        CHECK_ARG(chain_off, "select: null chain_off");
        CHECK_ARG(chain_off[0] == 0, "select: chain_off[0] must be 0");
        for (int64_t g = 0; g < ng; ++g)
            if (chain_off[g + 1] < chain_off[g])
                fail(BWTMI_E_ARG, "select: chain_off decreases at group %lld", (long long)g);
        const int64_t nc = chain_off[ng];
        CHECK_ARG(nc == 0 || score, "select: null score array");
        CHECK_ARG(nc == 0 || qstart, "select: null qstart array");
        CHECK_ARG(nc == 0 || qend, "select: null qend array");
        int32_t max_score = 0;
        for (int64_t i = 0; i < nc; ++i) {
            if (score[i] < 1 || score[i] > (1 << 30))
                fail(BWTMI_E_ARG, "select: score %d of chain %lld outside 1..2^30", (int)score[i], (long long)i);
            if (qstart[i] < 0) fail(BWTMI_E_ARG, "select: qstart %d of chain %lld is negative", (int)qstart[i], (long long)i);
            if (qend[i] <= qstart[i] || qend[i] > (1 << 28))
                fail(BWTMI_E_ARG, "select: qend %d of chain %lld outside qstart %d < qend <= 2^28", (int)qend[i],
                     (long long)i, (int)qstart[i]);
            max_score = std::max(max_score, score[i]);
        }
        SelectResult r;
        select_chains_device(use(ctx->c), chain_off, ng, score, qstart, qend, max_score, p, r);
        *parent = malloc_copy(r.parent);
        *sub = malloc_copy(r.sub);
        *mapq = malloc_copy(r.mapq);
        *keep = malloc_copy(r.keep);
        if (n_primary) *n_primary = r.n_primary;
        if (n_kept) *n_kept = r.n_kept;
    });
}

int bwtmi_index_align_chains(bwtmi_ctx *ctx, bwtmi_index *idx, const uint8_t *qs, const int64_t *off, int64_t nq,
                             const int64_t *chain_off, const uint8_t *strand, const int64_t *member_off,
                             const int32_t *member_q, const int64_t *member_r, const int32_t *member_len,
                             int64_t nchain, int64_t nmember, const bwtmi_align_params *params, int64_t **cigar_off,
                             uint32_t **cigar, int32_t **nm, int32_t **n_eq, int32_t **cols, int32_t **aq_start,
                             int32_t **aq_end, int64_t **ar_start, int64_t **ar_end, int64_t *ncigar,
                             int64_t *cells_total, int64_t *gaps) {
    return guard([&] {
        CHECK_ARG(ctx && idx && cigar_off && cigar && nm && n_eq && cols && aq_start && aq_end && ar_start && ar_end &&
                      ncigar,
                  "bad argument");
        *cigar_off = *ar_start = *ar_end = nullptr;
        *cigar = nullptr;
        *nm = *n_eq = *cols = *aq_start = *aq_end = nullptr;
        *ncigar = 0;
        if (cells_total) *cells_total = 0;
        if (gaps) gaps[0] = gaps[1] = gaps[2] = 0;
        AlignParams p;
        if (params) {
            CHECK_ARG(params->reserved[0] == 0 && params->reserved[1] == 0 && params->reserved[2] == 0,
                      "align: reserved fields must be 0");
            if (params->band >= 0) p.band = params->band;
            if (params->max_cells > 0) p.max_cells = params->max_cells;
        }
        AlignResult r;
        try {
            index_align_chains(use(ctx->c), idx->d, qs, off, nq, chain_off, strand, member_off, member_q, member_r,
                               member_len, nchain, nmember, p, r);
        } catch (...) {
            if (cells_total) *cells_total = r.cells_total;   // the count a tripped cap reports
            throw;
        }
        if (cells_total) *cells_total = r.cells_total;
        if (gaps) std::copy(r.gaps, r.gaps + 3, gaps);
        *cigar_off = malloc_copy(r.cigar_off);
        *cigar = malloc_copy(r.cigar);
        *nm = malloc_copy(r.nm);
        *n_eq = malloc_copy(r.n_eq);
        *cols = malloc_copy(r.cols);
        *aq_start = malloc_copy(r.aq_start);
        *aq_end = malloc_copy(r.aq_end);
        *ar_start = malloc_copy(r.ar_start);
        *ar_end = malloc_copy(r.ar_end);
        *ncigar = (int64_t)r.cigar.size();
    });
}

int bwtmi_index_align_extend(bwtmi_ctx *ctx, bwtmi_index *idx, const uint8_t *qs, const int64_t *off, int64_t nq,
                             const int64_t *chain_off, const uint8_t *strand, const int64_t *member_off,
                             const int32_t *member_q, const int64_t *member_r, const int32_t *member_len,
                             int64_t nchain, int64_t nmember, const bwtmi_extend_params *params, int64_t **cigar_off,
                             uint32_t **cigar, int32_t **nm, int32_t **n_eq, int32_t **cols, int32_t **aq_start,
                             int32_t **aq_end, int64_t **ar_start, int64_t **ar_end, int32_t **head_score,
                             int32_t **tail_score, int64_t *ncigar, int64_t *cells_total, int64_t *gaps,
                             int64_t *ext_rows) {
    return guard([&] {
        CHECK_ARG(ctx && idx && cigar_off && cigar && nm && n_eq && cols && aq_start && aq_end && ar_start && ar_end &&
                      head_score && tail_score && ncigar,
                  "bad argument");
        *cigar_off = *ar_start = *ar_end = nullptr;
        *cigar = nullptr;
        *nm = *n_eq = *cols = *aq_start = *aq_end = *head_score = *tail_score = nullptr;
        *ncigar = 0;
        if (cells_total) *cells_total = 0;
        if (gaps) gaps[0] = gaps[1] = gaps[2] = 0;
        if (ext_rows) *ext_rows = 0;
        AlignParams p;
        ExtendParams e;
        if (params) {
            CHECK_ARG(params->reserved[0] == 0 && params->reserved[1] == 0, "align: reserved fields must be 0");
            if (params->band >= 0) p.band = params->band;
            if (params->max_cells > 0) p.max_cells = params->max_cells;
            if (params->ext_band >= 0) e.ext_band = params->ext_band;
            if (params->match >= 0) e.match = params->match;
            if (params->mismatch >= 0) e.mismatch = params->mismatch;
            if (params->gap >= 0) e.gap = params->gap;
            if (params->xdrop >= 0) e.xdrop = params->xdrop;
        }
        AlignResult r;
        try {
            index_align_extend(use(ctx->c), idx->d, qs, off, nq, chain_off, strand, member_off, member_q, member_r,
                               member_len, nchain, nmember, p, e, r);
        } catch (...) {
            if (cells_total) *cells_total = r.cells_total;   // the count a tripped cap reports
            throw;
        }
        if (cells_total) *cells_total = r.cells_total;
        if (gaps) std::copy(r.gaps, r.gaps + 3, gaps);
        if (ext_rows) *ext_rows = r.ext_rows;
        *cigar_off = malloc_copy(r.cigar_off);
        *cigar = malloc_copy(r.cigar);
        *nm = malloc_copy(r.nm);
        *n_eq = malloc_copy(r.n_eq);
        *cols = malloc_copy(r.cols);
        *aq_start = malloc_copy(r.aq_start);
        *aq_end = malloc_copy(r.aq_end);
        *ar_start = malloc_copy(r.ar_start);
        *ar_end = malloc_copy(r.ar_end);
        *head_score = malloc_copy(r.head_score);
        *tail_score = malloc_copy(r.tail_score);
        *ncigar = (int64_t)r.cigar.size();
    });
}

static LibParams lib_params(const bwtmi_lib_params *p) {
    LibParams q;
    if (p) {
        q.min_period = p->min_period;
        q.max_period = p->max_period;
        q.max_short_motif = p->max_short_motif;
        q.min_copies = p->min_copies;
        q.min_array_length = p->min_array_length;
        q.allow_mismatches = p->allow_mismatches;
        q.min_entropy = p->min_entropy;
    }
    return q;
}

int bwtmi_index_lcp_plateaus(bwtmi_ctx *ctx, bwtmi_index *idx, const bwtmi_lib_params *p, int64_t **out,
                             int64_t *n) {
    return guard([&] {
        CHECK_ARG(ctx && idx && out && n, "null argument");
        *out = nullptr;
        *n = 0;
        use(ctx->c);
        std::vector<int64_t> v;
        lcp_plateaus_device(ctx->c, idx->d, lib_params(p), v);
        *out = malloc_copy(v);
        *n = (int64_t)(v.size() / 3);
    });
}

int bwtmi_index_short_imperfect(bwtmi_ctx *ctx, bwtmi_index *idx, const bwtmi_lib_params *p, const int64_t *seen,
                                int64_t nseen, bwtmi_job *job, int32_t contig_id) {
    return guard([&] {
        CHECK_ARG(ctx && idx && job && (seen || nseen == 0) && nseen >= 0, "bad argument");
        CHECK_ARG(contig_id >= 0 && contig_id < (int32_t)job->j.contigs.size(), "bad contig id");
        CHECK_ARG((int64_t)job->j.contigs[(size_t)contig_id].full.size() == index_n(idx->d),
                  "the job contig must hold the index text");
        use(ctx->c);
        std::vector<int64_t> sp(seen, seen + 2 * nseen);
        short_imperfect_device(ctx->c, idx->d, lib_params(p), sp, contig_id, job->j.recs_own());
        job->j.postprocessed = true;
    });
}

int bwtmi_index_tier3(bwtmi_ctx *ctx, bwtmi_index *idx, const uint8_t *reads, const int64_t *read_off,
                      int64_t nreads, bwtmi_job *job, int32_t contig_id, int32_t as_input) {
    return guard([&] {
        CHECK_ARG(ctx && idx && job && nreads >= 0 && (read_off || nreads == 0), "bad argument");
        CHECK_ARG(contig_id >= 0 && contig_id < (int32_t)job->j.contigs.size(), "bad contig id");
        if (nreads > 0) {
            CHECK_ARG(read_off[0] == 0 && (reads || read_off[nreads] == 0), "bad read offsets");
            for (int64_t r = 0; r < nreads; ++r) CHECK_ARG(read_off[r + 1] >= read_off[r], "bad read offsets");
        }
        use(ctx->c);
        RecVec recs;
        tier3_device(ctx->c, idx->d, reads, read_off, nreads, contig_id, recs);
        Job &J = job->j;
        if (as_input) {
            if (J.t3.size() < J.contigs.size()) J.t3.resize(J.contigs.size());
            auto &dst = J.t3[(size_t)contig_id];
            for (auto &r : recs) dst.push_back(std::move(r));
        } else {
            RecVec &fin = J.recs_own();
            for (auto &r : recs) fin.push_back(std::move(r));
            J.postprocessed = true;
        }
    });
}

int bwtmi_index_long_repeats(bwtmi_ctx *ctx, bwtmi_index *idx, const bwtmi_lib_params *p, const int64_t *seen,
                             int64_t nseen, bwtmi_job *job, int32_t contig_id) {
    return guard([&] {
        CHECK_ARG(ctx && idx && job && (seen || nseen == 0) && nseen >= 0, "bad argument");
        CHECK_ARG(contig_id >= 0 && contig_id < (int32_t)job->j.contigs.size(), "bad contig id");
        CHECK_ARG(p->min_copies >= 0 && p->min_array_length >= 0, "bad parameters");
        use(ctx->c);
        std::vector<int64_t> sp(seen, seen + 2 * nseen);
        simple_scan_device(ctx->c, idx->d, lib_params(p), sp, contig_id, job->j.recs_own());
        job->j.postprocessed = true;
    });
}

int bwtmi_job_tier1(bwtmi_ctx *ctx, bwtmi_job *job, int32_t contig_id, int32_t max_motif_length) {
    return guard([&] {
        CHECK_ARG(ctx && job, "null argument");
        TEXT_JOIN(job);
        CHECK_ARG(contig_id >= 0 && contig_id < (int32_t)job->j.contigs.size(), "bad contig id");
        Ctx &c = ctx->c;
        use(c);
        const Seq &full = job->j.contigs[(size_t)contig_id].full;
        const int64_t n = (int64_t)full.size();
        upload_text(c, c.slot[S_TEXT], (const uint8_t *)full.data(), n);
        tier1_device(c, c.slot[S_TEXT].as<uint8_t>(), (const uint8_t *)full.data(), n, max_motif_length, contig_id,
                     job->j.recs_own());
        job->j.postprocessed = true;
    });
}

// ------------------------------------------------------------ job
int bwtmi_job_create(const bwtmi_params *params, bwtmi_job **out) {
    return guard([&] {
        CHECK_ARG(params && out, "null argument");
        auto *j = new bwtmi_job();
        j->j.params = *params;
        if (j->j.params.sa_sample <= 0) j->j.params.sa_sample = 32;
        *out = j;
    });
}

int bwtmi_job_free(bwtmi_job *job) {
    return guard([&] {
        if (!job) return;
        if (job->j.text_th.joinable()) job->j.text_th.join();   // its error dies with the job
        if (job->wr) (void)job->wr->finish();   // a file still being written is finished (its error dies too)
        if (job->units_wr.joinable()) job->units_wr.join();
        if (job->dev.bg_ctx) ctx_join(*job->dev.bg_ctx);   // its error stays for the ctx's next call
        if (job->dev.device >= 0) (void)hipSetDevice(job->dev.device);
        for (auto &d : job->dev.seqs) d.buf.release();
        delete job;
    });
}

int bwtmi_job_add_contig(bwtmi_job *job, const char *name, const uint8_t *full, int64_t full_len,
                         int64_t trim_left, int64_t trim_right, int32_t *contig_id) {
    return guard([&] {
        CHECK_ARG(job && name && (full || full_len == 0) && full_len >= 0, "bad argument");
        TEXT_JOIN(job);
        CHECK_ARG(trim_left >= 0 && trim_right >= 0 && trim_left + trim_right <= full_len, "bad trim");
        job->j.recs_own();   // a new contig may renumber the fold units the survivors are kept by
        Contig c;
        c.name = name;
        c.full.assign((const char *)full, (size_t)full_len);
        c.trim_left = trim_left;
        c.trim_right = trim_right;
        c.weight = full_len - trim_left - trim_right;
        c.gen = next_contig_gen();
        job->j.contigs.push_back(std::move(c));
        if (contig_id) *contig_id = (int32_t)job->j.contigs.size() - 1;
    });
}

int bwtmi_job_load_fasta(bwtmi_job *job, const char *path, int32_t flank_trim) {
    return guard([&] {
        BWTMI_STAGE("bwtmi:load");
        CHECK_ARG(job && path, "null argument");
        TEXT_JOIN(job);
        load_fasta(job->j, path, flank_trim);
        pool_spin_for_job(job->j);
    });
}

// bwtmi_job_load_fasta_dev: the loader's device placement (common.h FastaDev).
// The file image goes up right after the read (pinned, overlapping the host's
// first pass), the plain chunks are rebuilt from it on the device
// (fasta_dev.hip), the host-written pieces follow, and the host pass over the
// plain chunks runs behind all of it (joined by the scan or any reader).
namespace {
struct DevLoad final : FastaDev {
    Ctx &c;
    bwtmi_job *job;
    DevLoad(Ctx &c_, bwtmi_job *j) : c(c_), job(j) {}
    const char *img = nullptr;
    bool preloaded = false;   // the image is the pass-1 part already queued to S_FASTA
    void image(const char *p, int64_t n) override {
        img = p;
        const Job &J = job->j;
        preloaded = J.part_dev_tag != 0 && c.fasta_tag == J.part_dev_tag && p == J.part.data() &&
                    n <= (int64_t)J.part.size();
        if (!preloaded) c.fasta_tag = 0;   // S_FASTA gets other bytes
        if (n <= 0 || preloaded) return;
        ensure_pinned(p, p, (size_t)n);
        c.slot[S_FASTA].ensure((size_t)n + 64);
    }
    void image_part(int64_t off, int64_t n) override {   // from the reading threads
        if (preloaded) return;
        HIPCHECK(hipSetDevice(c.device));
        HIPCHECK(hipMemcpyAsync(c.slot[S_FASTA].as<char>() + off, img + off, (size_t)n, hipMemcpyHostToDevice,
                                c.stream));
    }
    void contigs() override {
        JobDev &d = job->dev;
        const Job &J = job->j;
        d.rebind(c.device, J.contigs.size());
        for (size_t i = 0; i < J.contigs.size(); ++i) {
            const Contig &ct = J.contigs[i];
            DevContig &dc = d.seqs[i];
            if (!J.selected.empty() && (i >= J.selected.size() || !J.selected[i])) continue;   // another rank's contig
            const int64_t tn = ct.trimmed_len();
            if (dc.n == tn && dc.gen == ct.gen) continue;   // on the device already (not in this file)
            if (!ct.full.empty()) ensure_pinned(ct.full.data(), ct.full.data(), ct.full.size());
            dc.buf.ensure((size_t)tn + 128);
            HIPCHECK(hipMemsetAsync(dc.buf.as<uint8_t>() + tn, 0, 128, c.stream));
            dc.n = tn;
            dc.gen = ct.gen;
        }
    }
    void plain(const std::vector<FastaPiece> &ps) override {
        std::vector<FastaDevPiece> v;
        v.reserve(ps.size());
        for (const FastaPiece &p : ps) {
            const Contig &ct = job->j.contigs[(size_t)p.cid];
            v.push_back(FastaDevPiece{p.a, p.b, p.off, ct.trim_left, ct.trimmed_len(),
                                      job->dev.seqs[(size_t)p.cid].buf.as<char>()});
        }
        fasta_build_device(c, c.slot[S_FASTA].as<uint8_t>(), v.data(), (int64_t)v.size());
    }
    void piece(int32_t cid, int64_t off, const char *host, int64_t n) override {
        const Contig &ct = job->j.contigs[(size_t)cid];
        const int64_t tl = ct.trim_left, tn = ct.trimmed_len();
        const int64_t lo = std::max(off, tl), hi = std::min(off + n, tl + tn);
        if (hi <= lo) return;
        HIPCHECK(hipMemcpyAsync(job->dev.seqs[(size_t)cid].buf.as<char>() + (lo - tl), host + (lo - off),
                                (size_t)(hi - lo), hipMemcpyHostToDevice, c.stream));
    }
    void defer(std::function<void()> fn, std::shared_ptr<void> hold) override {
        hipEvent_t ev;   // every copy out of `hold` (the image) is queued before it
        HIPCHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIPCHECK(hipEventRecord(ev, c.stream));
        const int dev = c.device;
        job->j.text_defer([fn = std::move(fn), hold = std::move(hold), ev, dev]() mutable {
            struct Done {   // also when fn throws: the image outlives its copy
                hipEvent_t ev;
                int dev;
                std::shared_ptr<void> &hold;
                ~Done() {
                    (void)hipSetDevice(dev);
                    (void)hipEventSynchronize(ev);
                    (void)hipEventDestroy(ev);
                    hold.reset();
                }
            } done{ev, dev, hold};
            fn();
        });
    }
};
}  // namespace

int bwtmi_job_load_fasta_dev(bwtmi_ctx *ctx, bwtmi_job *job, const char *path, int32_t flank_trim) {
    return guard([&] {
        BWTMI_STAGE("bwtmi:load");
        CHECK_ARG(ctx && job && path, "null argument");
        Ctx &c = ctx->c;
        job->j.text_join();
        job_use(c, job);   // (another context's builds read the old buffers)
        device_wake(c);
        DevLoad dl(c, job);
        load_fasta(job->j, path, flank_trim, 1, 0, &dl);
        pool_spin_for_job(job->j);
    });
}

int bwtmi_job_device_text(bwtmi_ctx *ctx, bwtmi_job *job, int32_t id, uint8_t *dst) {
    return guard([&] {
        CHECK_ARG(ctx && job && dst && id >= 0 && id < (int32_t)job->j.contigs.size(), "bad argument");
        Ctx &c = use(ctx->c);
        const JobDev &d = job->dev;
        CHECK_ARG(d.device == c.device && (size_t)id < d.seqs.size() && d.seqs[(size_t)id].n >= 0 &&
                      d.seqs[(size_t)id].gen == job->j.contigs[(size_t)id].gen,
                  "contig not resident on this device");
        const DevContig &dc = d.seqs[(size_t)id];
        if (dc.n) HIPCHECK(hipMemcpyAsync(dst, dc.buf.p, (size_t)dc.n, hipMemcpyDeviceToHost, c.stream));
        HIPCHECK(hipStreamSynchronize(c.stream));
    });
}

int bwtmi_job_load_fasta_shard(bwtmi_job *job, const char *path, int32_t flank_trim, int32_t world, int32_t rank) {
    return guard([&] {
        BWTMI_STAGE("bwtmi:load");
        CHECK_ARG(job && path && world >= 1 && rank >= 0 && rank < world, "bad argument");
        TEXT_JOIN(job);
        load_fasta(job->j, path, flank_trim, world, rank);
        pool_spin_for_job(job->j);
    });
}

int bwtmi_job_fasta_scan_part(bwtmi_job *job, const char *path, int32_t world, int32_t rank, int64_t **blob,
                              int64_t *nwords) {
    return guard([&] {
        BWTMI_STAGE("bwtmi:load");
        CHECK_ARG(job && path && blob && nwords && world >= 1 && rank >= 0 && rank < world, "bad argument");
        TEXT_JOIN(job);
        std::vector<int64_t> v;
        fasta_scan_part(job->j, path, world, rank, v);
        *blob = malloc_copy(v);
        *nwords = (int64_t)v.size();
    });
}

// pass 1 as above, and the part's bytes queued to ctx's FASTA image slot right
// away: when this rank's contigs lie inside its part (equal contigs, one per
// rank), pass 2 (bwtmi_job_load_fasta_parts_dev on the same ctx) finds its
// image on the device and the copy has overlapped the part-table exchange
int bwtmi_job_fasta_scan_part_dev(bwtmi_ctx *ctx, bwtmi_job *job, const char *path, int32_t world, int32_t rank,
                                  int64_t **blob, int64_t *nwords) {
    return guard([&] {
        BWTMI_STAGE("bwtmi:load");
        CHECK_ARG(ctx && job && path && blob && nwords && world >= 1 && rank >= 0 && rank < world, "bad argument");
        TEXT_JOIN(job);
        Ctx &c = ctx->c;
        job_use(c, job);
        // the previous part's copy (if any, on whichever context) has left
        // job->j.part before pass 1 overwrites it (fasta_scan_part settles it)
        std::vector<int64_t> v;
        fasta_scan_part(job->j, path, world, rank, v);
        const Seq &part = job->j.part;
        if (!part.empty()) {
            static std::atomic<uint64_t> tags{0};
            const uint64_t tag = ++tags;
            ensure_pinned(part.data(), part.data(), part.size());
            c.slot[S_FASTA].ensure(part.size() + 64);
            HIPCHECK(hipMemcpyAsync(c.slot[S_FASTA].p, part.data(), part.size(), hipMemcpyHostToDevice, c.stream));
            hipEvent_t ev;
            HIPCHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            HIPCHECK(hipEventRecord(ev, c.stream));
            job->j.part_inflight = [ev] {   // an event wait needs no current device
                (void)hipEventSynchronize(ev);
                (void)hipEventDestroy(ev);
            };
            c.fasta_tag = tag;
            job->j.part_dev_tag = tag;
        }
        *blob = malloc_copy(v);
        *nwords = (int64_t)v.size();
    });
}

int64_t bwtmi_fasta_count_records(const char *path, int64_t limit) {
    if (!path || limit < 0) return -1;
    try {
        return fasta_count_records(path, limit);
    } catch (...) {
        return -1;
    }
}

int bwtmi_job_load_fasta_parts_dev(bwtmi_ctx *ctx, bwtmi_job *job, const char *path, int32_t flank_trim,
                                   int32_t world, int32_t rank, const int64_t *blob, int64_t nwords) {
    return guard([&] {
        BWTMI_STAGE("bwtmi:load");
        CHECK_ARG(ctx && job && path && blob && nwords >= 6 && world >= 1 && rank >= 0 && rank < world,
                  "bad argument");
        Ctx &c = ctx->c;
        job->j.text_join();
        job_use(c, job);
        device_wake(c);
        DevLoad dl(c, job);
        fasta_load_parts(job->j, path, flank_trim, world, rank, blob, nwords, &dl);
        pool_spin_for_job(job->j);
    });
}

int bwtmi_job_load_fasta_parts(bwtmi_job *job, const char *path, int32_t flank_trim, int32_t world, int32_t rank,
                               const int64_t *blob, int64_t nwords) {
    return guard([&] {
        BWTMI_STAGE("bwtmi:load");
        CHECK_ARG(job && path && blob && nwords >= 6 && world >= 1 && rank >= 0 && rank < world, "bad argument");
        TEXT_JOIN(job);
        fasta_load_parts(job->j, path, flank_trim, world, rank, blob, nwords);
        pool_spin_for_job(job->j);
    });
}

int bwtmi_job_select_shard(bwtmi_job *job, int32_t world, int32_t rank, int32_t *ids, int32_t *n) {
    return guard([&] {
        CHECK_ARG(job && world >= 1 && rank >= 0 && rank < world, "bad argument");
        TEXT_JOIN(job);
        std::vector<int32_t> v = shard_units(job->j, world, rank);
        Job &J = job->j;
        J.selected.assign(J.contigs.size(), 0);
        for (int32_t c : v) J.selected[(size_t)c] = 1;
        if (n) *n = (int32_t)v.size();
        if (ids) std::copy(v.begin(), v.end(), ids);
    });
}

int bwtmi_host_info(int32_t *cpus_visible, int32_t *local_world, int32_t *threads) {
    return guard([&] {
        int v = 0, lw = 0;
        const int t = host_cpu_budget(&v, &lw);
        if (cpus_visible) *cpus_visible = v;
        if (local_world) *local_world = lw;
        if (threads) *threads = t;
    });
}

int32_t bwtmi_job_contig_count(const bwtmi_job *job) { return job ? (int32_t)job->j.contigs.size() : -1; }

int64_t bwtmi_job_contig_weight(const bwtmi_job *job, int32_t id) {
    if (!job || id < 0 || id >= (int32_t)job->j.contigs.size()) return -1;
    return job->j.contigs[(size_t)id].weight;
}

int64_t bwtmi_job_contig_info(const bwtmi_job *job, int32_t id, char *name, int64_t cap, int64_t *full_len,
                              int64_t *trim_left, int64_t *trim_right) {
    if (!job || id < 0 || id >= (int32_t)job->j.contigs.size()) return -1;
    const Contig &c = job->j.contigs[(size_t)id];
    if (name && cap > 0) {
        const size_t k = std::min<size_t>((size_t)cap - 1, c.name.size());
        std::memcpy(name, c.name.data(), k);
        name[k] = 0;
    }
    if (full_len) *full_len = (int64_t)c.full.size();
    if (trim_left) *trim_left = c.trim_left;
    if (trim_right) *trim_right = c.trim_right;
    return (int64_t)c.name.size();
}

int bwtmi_job_contig_seq(const bwtmi_job *job, int32_t id, uint8_t *dst) {
    return guard([&] {
        CHECK_ARG(job && dst && id >= 0 && id < (int32_t)job->j.contigs.size(), "bad argument");
        TEXT_JOIN(job);
        const Contig &c = job->j.contigs[(size_t)id];
        std::memcpy(dst, c.full.data(), c.full.size());
    });
}

static void job_upload(bwtmi_ctx *ctx, bwtmi_job *job) {
    Ctx &c = ctx->c;
    job_use(c, job);
    JobDev &d = job->dev;
    d.rebind(c.device, job->j.contigs.size());
    for (size_t i = 0; i < job->j.contigs.size(); ++i) {
        const Contig &ct = job->j.contigs[i];
        DevContig &dc = d.seqs[i];
        if (!job->j.selected.empty() && !job->j.selected[i]) continue;   // another rank's shard
        if (dc.n == ct.trimmed_len() && dc.gen == ct.gen) continue;
        job->j.text_join();   // host bytes are read below
        ensure_pinned(ct.full.data(), ct.trimmed(), (size_t)ct.trimmed_len());
        upload_text(c, dc.buf, (const uint8_t *)ct.trimmed(), ct.trimmed_len());
        dc.n = ct.trimmed_len();
        dc.gen = ct.gen;
    }
    HIPCHECK(hipStreamSynchronize(c.stream));
}

int bwtmi_job_upload(bwtmi_ctx *ctx, bwtmi_job *job) {
    return guard([&] {
        BWTMI_STAGE("bwtmi:upload");
        CHECK_ARG(ctx && job, "null argument");
        job_upload(ctx, job);
    });
}

int bwtmi_job_reset(bwtmi_job *job) {
    return guard([&] {
        CHECK_ARG(job, "null argument");
        job->j.hits.clear();
        job->j.screened.clear();
        job->j.shits.clear();
        job->j.raw_n.clear();
        job->j.drop_results();   // released on the background reaper thread, behind the next step's device phase
        job->j.t3.clear();
        job->j.postprocessed = false;
    });
}

int bwtmi_job_set_params(bwtmi_job *job, const bwtmi_params *params) {
    return guard([&] {
        CHECK_ARG(job && params, "null argument");
        job->j.params = *params;
        if (job->j.params.sa_sample <= 0) job->j.params.sa_sample = 32;
    });
}

int bwtmi_job_select(bwtmi_job *job, const int32_t *ids, int32_t n) {
    return guard([&] {
        CHECK_ARG(job && (ids || n <= 0), "bad argument");
        Job &J = job->j;
        J.selected.clear();
        if (n < 0) return;
        J.selected.assign(J.contigs.size(), 0);
        for (int32_t k = 0; k < n; ++k) {
            CHECK_ARG(ids[k] >= 0 && ids[k] < (int32_t)J.contigs.size(), "bad contig id");
            J.selected[(size_t)ids[k]] = 1;
        }
    });
}

// ------------------------------------------------------------ scan
extern "C++" {
namespace {
using DevText = std::pair<const uint8_t *, int64_t>;   // a contig's device copy and its length

// what one bwtmi_job_scan does (scan_plan)
struct ScanPlan {
    std::vector<size_t> todo;         // contigs to scan
    std::vector<DevText> to_index;    // contigs to index
    std::vector<int32_t> unit_size;   // contigs per fold unit
    // nested suppression + sort + dedup on the device (BWTMI_HOST_SCREEN=1: on the host)
    bool screen = knob(KN_HOST_SCREEN) == 0;
    const char *fail_contig = std::getenv("BWTMI_FAIL_CONTIG");   // test hook: this contig's worker fails
    const char *fail_kind = std::getenv("BWTMI_FAIL_KIND");       // "hip": as a device fault
};

// The job's last results are cleared; which of its (uploaded) contigs are
// scanned and indexed, and the sizes of their fold units.
ScanPlan scan_plan(bwtmi_job *job) {
    Job &J = job->j;
    J.hits.assign(J.contigs.size(), {});
    J.screened.assign(J.contigs.size(), 0);
    J.shits.assign(J.contigs.size(), {});
    J.raw_n.assign(J.contigs.size(), 0);
    J.errors.assign(J.contigs.size(), std::string());
    J.drop_results();
    J.postprocessed = false;
    ScanPlan plan;
    const bwtmi_params &P = J.params;
    for (size_t i = 0; i < J.contigs.size(); ++i) {
        const int64_t len = J.contigs[i].trimmed_len();
        if (!J.selected.empty() && !J.selected[i]) continue;   // another rank's shard
        if (P.build_index) plan.to_index.push_back({job->dev.seqs[i].buf.as<uint8_t>(), len});
        if (!P.tier2) continue;                                  // bwt.py:3068
        if (len > 50000000 && !P.show_progress) continue;        // bwt.py:3070
        if (P.min_copies <= 0) continue;                         // worker raises -> [] (bwt.py:3137)
        plan.todo.push_back(i);
    }
    // the screen drops hits only the final filter would see (nested.hip) for a
    // contig that is a fold unit of its own: in a unit of several contigs the
    // records interleave by position, and another contig's record between two
    // breaks their merge chain (bwt.py:3222-3289)
    J.assign_units();
    plan.unit_size.assign((size_t)std::max<int32_t>(1, J.nunits), 0);
    for (const Contig &ct : J.contigs) ++plan.unit_size[(size_t)ct.unit];
    return plan;
}

// the strict scan of contig i on context lc (c or one of its lanes)
void scan_contig(Ctx &lc, bwtmi_job *job, const ScanPlan &plan, size_t i) {
    Job &J = job->j;
    const bwtmi_params &P = J.params;
    const Contig &ct = J.contigs[i];
    const int64_t len = ct.trimmed_len();
    const int64_t U = std::max<int64_t>(P.max_unit_len, std::min<int64_t>(len / P.min_copies, 1000));
    // a contig with Tier 3 records is screened on the host, together with them
    const bool t3 = i < J.t3.size() && !J.t3[i].empty();
    ScanResult r;
    // a failing contig yields no records and an error message, the others go on
    // (the worker's `except Exception: print(...); return []`, bwt.py:3137-3141)
    // A device fault (BWTMI_E_HIP: a failed launch, copy or synchronisation) is
    // not contig-local -- the lanes share one device, and a sticky fault fails
    // every later contig -- and the reference has no such failure: the scan
    // stops and the call returns the error, so the run fails instead of
    // writing a partial repeat.tab.
    try {
        if (plan.fail_contig && ct.name == plan.fail_contig)
            fail(plan.fail_kind && !std::strcmp(plan.fail_kind, "hip") ? BWTMI_E_HIP : BWTMI_E_STATE,
                 "injected failure (BWTMI_FAIL_CONTIG)");
        strict_scan_device(lc, job->dev.seqs[i].buf.as<uint8_t>(), len, 1, (int32_t)std::min<int64_t>(U, INT32_MAX),
                           P.min_copies, r, plan.screen && !t3 && len < (int64_t)UINT32_MAX,   // 32-bit hit lengths
                           plan.unit_size[(size_t)ct.unit] == 1 ? P.min_copies : 0);
    } catch (const Error &e) {
        if (e.code == BWTMI_E_HIP) throw;
        J.errors[i] = e.msg;
        (void)hipGetLastError();
        (void)hipStreamSynchronize(lc.stream);
        return;
    } catch (const std::bad_alloc &) {
        J.errors[i] = "out of host memory";
        return;
    }
    J.hits[i].swap(r.hits);   // Rule 1 (bwt.py:3118-3130) never fires on strict hits
    J.shits[i].swap(r.shits);
    J.screened[i] = r.screened ? 1 : 0;
    J.raw_n[i] = r.raw;
}

// one index build on context x (its own stream, slots and scratch index)
void index_contig(Ctx &x, const DevText &tx, int32_t sa_sample) {
    const int64_t len = tx.second;
    // (S_CAND_K2 is free after the scan; index_build_device uses the MISC/IDX slots)
    DBuf &tb = x.slot[S_CAND_K2];
    tb.ensure((size_t)len + 1 + 128);
    HIPCHECK(hipMemcpyAsync(tb.p, tx.first, (size_t)len, hipMemcpyDeviceToDevice, x.stream));
    HIPCHECK(hipMemsetAsync(tb.as<uint8_t>() + len, '$', 1, x.stream));
    HIPCHECK(hipMemsetAsync(tb.as<uint8_t>() + len + 1, 0, 127, x.stream));
    x.scratch_index = index_build_device(x, tb.as<uint8_t>(), len + 1, sa_sample, 128, 0u, x.scratch_index);
}

size_t lanes_knob(Knob k) { return (size_t)std::clamp<int64_t>(knob(k), 1, 8); }

// The device lanes of c: fn(lane, i) for every item i < weights.size(), on nl
// contexts at once -- lane 0 is c on the calling thread, lane k >= 1 a context
// of its own (scan_lane: own stream and scratch) driven by its own host thread.
// A contig's scan or index build is a chain of small dependent launches and
// host reads, so one stream leaves the device idle between them.  Items go to
// lanes by lpt_assign and run longest first.  Every thread is joined before the
// first error (in lane order) is rethrown; a lane stops at its first error.
// At most one lane per item; one lane: the items in their order on c, no threads.
template <class F>
void run_lanes(Ctx &c, size_t nl, const std::vector<int64_t> &weights, F &&fn) {
    nl = std::min(nl, weights.size());
    if (nl <= 1) {
        for (size_t i = 0; i < weights.size(); ++i) fn(c, i);
        return;
    }
    const std::vector<size_t> owner = lpt_assign(weights, nl);
    std::vector<std::vector<size_t>> part(nl);
    for (size_t i = 0; i < owner.size(); ++i) part[owner[i]].push_back(i);
    for (auto &p : part)
        std::stable_sort(p.begin(), p.end(), [&](size_t x, size_t y) { return weights[x] > weights[y]; });
    std::vector<Ctx *> lc(nl);
    lc[0] = &c;
    for (size_t k = 1; k < nl; ++k) lc[k] = &scan_lane(c, k);
    std::vector<std::exception_ptr> ex(nl);
    auto run = [&](size_t k) {
        try {
            if (k) lc[k]->activate();
            for (size_t i : part[k]) fn(*lc[k], i);
        } catch (...) {
            ex[k] = std::current_exception();
        }
    };
    std::vector<std::thread> th;
    for (size_t k = 1; k < nl; ++k) th.emplace_back(run, k);
    run(0);
    for (auto &t : th) t.join();
    for (size_t k = 1; k < nl; ++k) c.absorb_kstats(*lc[k]);
    for (auto &e : ex)
        if (e) std::rethrow_exception(e);
}

// BWTCore(seq + '$') of the worker (bwt.py:3053-3054).  The worker never consumes
// it, so the builds run on the background thread c.bg behind the
// host post-processing.  The scratch index keeps its buffers between builds.
//
// Who may touch the context: while c.bg runs it owns c.stream, c.slot[],
// c.scratch_index, c.kstats / c.pending and every lane of c.  Every entry point
// reaches a context through use(), which joins c.bg first (ctx_wait) and
// rethrows its error.  job->dev.bg_ctx and c.bg_link are the two ends of one
// link -- the job names the context whose builds read its device buffers, the
// context names that job field -- so that either may end first: the job joins
// the context before it frees the buffers (bwtmi_job_free, job_use from
// another context), and the context's join clears the job's field (ctx_join).
void start_index_builds(Ctx &c, bwtmi_job *job, std::vector<DevText> to_index) {
    const int32_t sa_sample = job->j.params.sa_sample;
    c.bg_ms = 0;
    job->dev.bg_ctx = &c;
    c.bg_link = &job->dev.bg_ctx;
    c.bg = std::thread([&c, sa_sample, to_index = std::move(to_index)] {
        BWTMI_STAGE("bwtmi:index");
        auto ti = std::chrono::steady_clock::now();
        try {
            c.activate();
            // several contigs: the builds go to the lanes, each lane's builds on its
            // own stream and host thread -- a 12.5 Mbp build leaves the device mostly
            // idle, and eight of them in a row outlasted the host stages of the
            // 8-contig step (C4: 35 ms, r04final)
            const size_t nl = std::min<size_t>(lanes_knob(KN_INDEX_LANES), to_index.size());
            std::vector<int64_t> len;
            for (const DevText &tx : to_index) len.push_back(tx.second);
            run_lanes(c, nl, len, [&](Ctx &x, size_t i) { index_contig(x, to_index[i], sa_sample); });
            HIPCHECK(hipStreamSynchronize(c.stream));   // every lane's last build is done
            for (size_t k = 1; k < nl; ++k) HIPCHECK(hipStreamSynchronize(c.lanes[k - 1]->stream));
        } catch (const Error &e) {
            c.bg_code = e.code;
            c.bg_err = "background index build: " + e.msg;
        } catch (const std::bad_alloc &) {
            c.bg_code = BWTMI_E_NOMEM;
            c.bg_err = "background index build: out of host memory";
        } catch (const std::exception &e) {
            c.bg_code = BWTMI_E_STATE;
            c.bg_err = std::string("background index build: ") + e.what();
        }
        c.bg_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ti).count();
    });
}
}  // namespace
}  // extern "C++"

int bwtmi_job_scan(bwtmi_ctx *ctx, bwtmi_job *job) {
    return guard([&] {
        BWTMI_STAGE("bwtmi:scan");
        CHECK_ARG(ctx && job, "null argument");
        pool_spin_for_job(job->j);
        auto t0 = std::chrono::steady_clock::now();
        job_upload(ctx, job);
        Job &J = job->j;
        Ctx &c = ctx->c;
        ScanPlan plan = scan_plan(job);
        // several contigs: up to BWTMI_SCAN_LANES scans in flight (run_lanes)
        std::vector<int64_t> len;
        for (size_t i : plan.todo) len.push_back(J.contigs[i].trimmed_len());
        run_lanes(c, lanes_knob(KN_SCAN_LANES), len,
                  [&](Ctx &lc, size_t k) { scan_contig(lc, job, plan, plan.todo[k]); });
        J.text_join();   // the host copies written behind this scan (bwtmi_job_load_fasta_dev)
        J.stage_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        J.stage_ms[1] = 0;
        // every later use of this ctx (or of this job's device buffers) joins the builds first
        if (!plan.to_index.empty()) start_index_builds(c, job, std::move(plan.to_index));
    });
}

int bwtmi_job_wait(bwtmi_ctx *ctx, bwtmi_job *job) {
    return guard([&] {
        BWTMI_STAGE("bwtmi:index_wait");
        CHECK_ARG(ctx && job, "null argument");
        const bool ran = ctx->c.bg.joinable();
        ctx_wait(ctx->c);
        if (ran) job->j.stage_ms[1] = ctx->c.bg_ms;
    });
}

int bwtmi_job_add_hits(bwtmi_job *job, int32_t contig_id, const bwtmi_hit *hits, int64_t n) {
    return guard([&] {
        CHECK_ARG(job && (hits || n == 0) && n >= 0, "bad argument");
        TEXT_JOIN(job);
        Job &J = job->j;
        CHECK_ARG(contig_id >= 0 && contig_id < (int32_t)J.contigs.size(), "bad contig id");
        if (J.hits.size() < J.contigs.size()) J.hits.resize(J.contigs.size());
        if (J.screened.size() < J.contigs.size()) J.screened.resize(J.contigs.size(), 0);
        if (J.raw_n.size() < J.contigs.size()) J.raw_n.resize(J.contigs.size(), 0);
        CHECK_ARG(!J.screened[(size_t)contig_id] || n == 0,
                  "contig holds device-screened hits; reset the job before adding raw hits");
        J.hits[(size_t)contig_id].insert(J.hits[(size_t)contig_id].end(), hits, hits + n);
        J.raw_n[(size_t)contig_id] += n;
    });
}

int64_t bwtmi_job_raw_count(const bwtmi_job *job) {
    if (!job) return -1;
    int64_t n = 0;
    for (auto v : job->j.raw_n) n += v;
    return n;
}

int bwtmi_job_postprocess(bwtmi_job *job) {
    return guard([&] {
        BWTMI_STAGE("bwtmi:postprocess");
        CHECK_ARG(job, "null argument");
        pool_spin_for_job(job->j);
        TEXT_JOIN(job);
        Job &J = job->j;
        postprocess(J);
    });
}

int64_t bwtmi_job_count(const bwtmi_job *job) { return job ? (int64_t)job->j.count() : -1; }

int bwtmi_job_render(bwtmi_job *job, int fmt, char **out, int64_t *len) {
    return guard([&] {
        BWTMI_STAGE("bwtmi:write");
        CHECK_ARG(job && out && len, "null argument");
        pool_spin_for_job(job->j);
        TEXT_JOIN(job);
        const std::vector<Text> parts = render_parts(job->j, fmt);
        std::vector<size_t> at(parts.size() + 1, 0);
        for (size_t k = 0; k < parts.size(); ++k) at[k + 1] = at[k] + parts[k].size();
        const size_t tot = at.back();
        char *p = (char *)std::malloc(tot + 1);
        if (!p) fail(BWTMI_E_NOMEM, "malloc");
        run_tasks((int64_t)parts.size(), host_threads(job->j.params), [&](int64_t k) {
            std::memcpy(p + at[(size_t)k], parts[(size_t)k].data(), parts[(size_t)k].size());
        });
        p[tot] = 0;
        *out = p;
        *len = (int64_t)tot;
    });
}

// The file is written while it is being formatted (FileWrite): a part whose
// predecessors are all formatted has a known offset, and the writer thread
// writes each run of such parts as it completes.
int bwtmi_job_write(bwtmi_job *job, int fmt, const char *path) {
    return guard([&] {
        BWTMI_STAGE("bwtmi:write");
        CHECK_ARG(job && path, "null argument");
        write_join(job);
        write_start(job, fmt, path);
        write_join(job);
    });
}

// The same, returning once every row is formatted: the writer finishes the
// file behind the caller.  bwtmi_job_write_join waits for it and returns its
// error; every later write of the job, and bwtmi_job_free, joins it first.
int bwtmi_job_write_async(bwtmi_job *job, int fmt, const char *path) {
    return guard([&] {
        BWTMI_STAGE("bwtmi:write");
        CHECK_ARG(job && path, "null argument");
        write_join(job);
        write_start(job, fmt, path);
    });
}

int bwtmi_job_write_join(bwtmi_job *job) {
    return guard([&] {
        BWTMI_STAGE("bwtmi:write_join");
        CHECK_ARG(job, "null argument");
        write_join(job);
    });
}

int32_t bwtmi_job_unit_count(bwtmi_job *job) {
    if (!job) return -1;
    job->j.assign_units();
    return job->j.nunits;
}

int bwtmi_job_unit_rows(bwtmi_job *job, int64_t *unit_rows) {
    return guard([&] {
        CHECK_ARG(job && unit_rows, "null argument");
        TEXT_JOIN(job);
        Job &J = job->j;
        J.assign_units();
        for (int32_t u = 0; u < J.nunits; ++u) unit_rows[u] = 0;
        if (const std::shared_ptr<Survivors> sv = J.survivors()) {   // they know their units
            for (size_t k = 0; k < sv->units(); ++k) unit_rows[sv->unit_id(k)] = (int64_t)sv->unit_size(k);
            return;
        }
        for (const Rec &r : J.recs()) ++unit_rows[J.contigs[(size_t)r.chrom].unit];
    });
}

int bwtmi_job_render_units(bwtmi_job *job, int fmt, const int64_t *row_base, int64_t *bytes) {
    return guard([&] {
        BWTMI_STAGE("bwtmi:write");
        CHECK_ARG(job && bytes, "null argument");
        pool_spin_for_job(job->j);
        TEXT_JOIN(job);
        Job &J = job->j;
        render_rows(J, fmt, row_base, J.rendered);
        for (int32_t u = 0; u <= J.nunits; ++u) bytes[u] = 0;
        bytes[0] = (int64_t)J.rendered.header.size();
        for (size_t k = 0; k < J.rendered.parts.size(); ++k)
            bytes[1 + J.rendered.part_unit[k]] += (int64_t)J.rendered.parts[k].size();
    });
}

namespace {
// the rendered units (bwtmi_job_render_units) as parts at their file offsets;
// the job's rendering is handed over to them
void units_parts(bwtmi_job *job, const int64_t *offsets, int write_header, std::vector<Text> &parts,
                 std::vector<size_t> &at) {
    Job &J = job->j;
    Rendered &R = J.rendered;
    std::vector<int64_t> fill((size_t)J.nunits, 0);
    if (write_header && !R.header.empty()) {
        parts.emplace_back(R.header.data(), R.header.size());
        at.push_back((size_t)offsets[0]);
    }
    for (size_t k = 0; k < R.parts.size(); ++k) {
        const int32_t u = R.part_unit[k];
        at.push_back((size_t)(offsets[1 + u] + fill[(size_t)u]));
        fill[(size_t)u] += (int64_t)R.parts[k].size();
        parts.push_back(std::move(R.parts[k]));
    }
    R = Rendered();
}
}  // namespace

int bwtmi_job_write_units(bwtmi_job *job, const char *path, const int64_t *offsets, int write_header) {
    return guard([&] {
        BWTMI_STAGE("bwtmi:write");
        CHECK_ARG(job && path && offsets, "null argument");
        pool_spin_for_job(job->j);
        TEXT_JOIN(job);
        write_join(job);
        std::vector<Text> parts;
        std::vector<size_t> at;
        units_parts(job, offsets, write_header, parts, at);
        pwrite_parts(path, false, parts, at);
    });
}

// The same behind the caller: the parts are written by the job's own thread;
// bwtmi_job_write_join waits for it and returns its error (the job's next
// write and bwtmi_job_free join it first).
int bwtmi_job_write_units_async(bwtmi_job *job, const char *path, const int64_t *offsets, int write_header) {
    return guard([&] {
        BWTMI_STAGE("bwtmi:write");
        CHECK_ARG(job && path && offsets, "null argument");
        TEXT_JOIN(job);
        write_join(job);
        std::vector<Text> parts;
        std::vector<size_t> at;
        units_parts(job, offsets, write_header, parts, at);
        job->units_wr = std::thread([job, p = std::string(path), parts = std::move(parts), at = std::move(at)] {
            try {
                pwrite_parts(p.c_str(), false, parts, at);
            } catch (...) {
                job->units_err = std::current_exception();
            }
        });
    });
}

int bwtmi_job_get_records(bwtmi_job *job, int64_t *ints9, double *dbls5) {
    return guard([&] {
        CHECK_ARG(job && ints9 && dbls5, "null argument");
        TEXT_JOIN(job);
        size_t k = 0;
        for (const Rec &r : job->j.recs()) {
            int64_t *I = ints9 + 9 * k;
            double *D = dbls5 + 5 * k;
            I[0] = r.start; I[1] = r.end; I[2] = r.length; I[3] = r.tier; I[4] = r.n_eval; I[5] = r.max_mm;
            I[6] = r.score; I[7] = (r.stats_none ? 1 : 0) | (r.kmer_stats ? 2 : 0); I[8] = r.chrom;
            D[0] = r.copies; D[1] = r.mismatch_rate; D[2] = r.confidence; D[3] = r.pmatch; D[4] = r.pindel;
            ++k;
        }
    });
}

namespace {
// string `which` of a record (bwtmi_job_get_string); false for an unknown `which`
bool rec_string(const bwtmi_job *job, const Rec &r, int which, std::string_view &s) {
    switch (which) {
        case 0: case 1: s = r.motif; return true;
        case 2: s = r.variations; return true;
        case 3:
            s = {};
            if (r.act_kind != ACT_NONE) {
                const Contig &c = job->j.contigs[(size_t)r.chrom];
                const char *p = (r.act_kind == ACT_FULL ? c.full.data() : c.trimmed()) + r.act_off;
                s = std::string_view(p, (size_t)r.act_len);
            }
            return true;
        case 4: s = std::string_view(&r.strand, 1); return true;
        default: return false;
    }
}
}  // namespace

int64_t bwtmi_job_get_string(bwtmi_job *job, int64_t i, int which, char *buf, int64_t cap) {
    if (!job || i < 0 || i >= (int64_t)job->j.count()) return -1;
    std::string_view s;
    const Rec *r = nullptr;
    if (guard([&] { r = &job->j.recs()[(size_t)i]; }) != BWTMI_OK) return -1;
    if (!rec_string(job, *r, which, s)) return -1;
    if (buf && cap > 0) std::memcpy(buf, s.data(), std::min<size_t>((size_t)cap, s.size()));
    return (int64_t)s.size();
}

int64_t bwtmi_job_get_strings(bwtmi_job *job, int which, char *buf, int64_t cap, int64_t *offsets) {
    if (!job || which < 0 || which > 4) return -1;
    int64_t tot = 0;
    std::string_view s;
    const RecVec *built = nullptr;
    if (guard([&] { built = &job->j.recs(); }) != BWTMI_OK) return -1;
    const RecVec &recs = *built;
    for (size_t i = 0; i < recs.size(); ++i) {
        if (offsets) offsets[i] = tot;
        rec_string(job, recs[i], which, s);
        tot += (int64_t)s.size();
    }
    if (offsets) offsets[recs.size()] = tot;
    if (buf && cap >= tot) {
        char *w = buf;
        for (const Rec &r : recs) {
            rec_string(job, r, which, s);
            std::memcpy(w, s.data(), s.size());
            w += s.size();
        }
    }
    return tot;
}

// record wire format for the multi-GPU gather: POD header + strings
struct WireRec {
    int32_t chrom, tier;
    int64_t start, end, length, max_mm, n_eval, score, act_off, act_len;
    double copies, confidence, mismatch_rate, pmatch, pindel;
    int8_t act_kind, strand, is_compound, kmer_stats, stats_none;
    int32_t motif_len, var_len;
};

int bwtmi_job_export(bwtmi_job *job, uint8_t **buf, int64_t *len) {
    return guard([&] {
        CHECK_ARG(job && buf && len, "null argument");
        TEXT_JOIN(job);
        std::string s;
        const RecVec &recs = job->j.recs();
        const int64_t n = (int64_t)recs.size();
        s.append((const char *)&n, sizeof n);
        for (const Rec &r : recs) {
            WireRec w{};
            w.chrom = r.chrom; w.tier = r.tier; w.start = r.start; w.end = r.end; w.length = r.length;
            w.max_mm = r.max_mm; w.n_eval = r.n_eval; w.score = r.score; w.act_off = r.act_off; w.act_len = r.act_len;
            w.copies = r.copies; w.confidence = r.confidence; w.mismatch_rate = r.mismatch_rate;
            w.pmatch = r.pmatch; w.pindel = r.pindel; w.act_kind = r.act_kind; w.strand = r.strand;
            w.is_compound = r.is_compound; w.kmer_stats = r.kmer_stats; w.stats_none = r.stats_none;
            w.motif_len = (int32_t)r.motif.size(); w.var_len = (int32_t)r.variations.size();
            s.append((const char *)&w, sizeof w);
            s.append(r.motif);
            s.append(r.variations);
        }
        auto *p = (uint8_t *)std::malloc(s.size());
        if (!p) fail(BWTMI_E_NOMEM, "malloc");
        std::memcpy(p, s.data(), s.size());
        *buf = p;
        *len = (int64_t)s.size();
    });
}

static void import_wire(bwtmi_job *job, const uint8_t *buf, int64_t len) {
    CHECK_ARG(job && buf && len >= 8, "bad argument");
    RecVec &fin = job->j.recs_own();
    int64_t n;
    std::memcpy(&n, buf, 8);
    int64_t o = 8;
    for (int64_t k = 0; k < n; ++k) {
        CHECK_ARG(o + (int64_t)sizeof(WireRec) <= len, "truncated record buffer");
        WireRec w;
        std::memcpy(&w, buf + o, sizeof w);
        o += sizeof w;
        CHECK_ARG(w.motif_len >= 0 && w.var_len >= 0 && o + w.motif_len + w.var_len <= len, "truncated record strings");
        CHECK_ARG(w.chrom >= 0 && w.chrom < (int32_t)job->j.contigs.size(), "record for unknown contig");
        if (w.act_kind != ACT_NONE) {
            const Contig &c = job->j.contigs[(size_t)w.chrom];
            const int64_t L = w.act_kind == ACT_FULL ? (int64_t)c.full.size() : c.trimmed_len();
            CHECK_ARG(w.act_off >= 0 && w.act_len >= 0 && w.act_off + w.act_len <= L, "actual_sequence outside its contig");
        }
        Rec r;
        r.chrom = w.chrom; r.tier = w.tier; r.start = w.start; r.end = w.end; r.length = w.length;
        r.max_mm = w.max_mm; r.n_eval = w.n_eval; r.score = w.score; r.act_off = w.act_off; r.act_len = w.act_len;
        r.copies = w.copies; r.confidence = w.confidence; r.mismatch_rate = w.mismatch_rate;
        r.pmatch = w.pmatch; r.pindel = w.pindel; r.act_kind = w.act_kind; r.strand = (char)w.strand;
        r.is_compound = w.is_compound; r.kmer_stats = w.kmer_stats; r.stats_none = w.stats_none;
        r.motif.assign((const char *)buf + o, (size_t)w.motif_len);
        o += w.motif_len;
        r.variations.assign((const char *)buf + o, (size_t)w.var_len);
        o += w.var_len;
        fin.push_back(std::move(r));
    }
    // keep the reference's global order (natural chrom, start, end; stable,
    // bwt.py:3184-3187, 4147): every unit arrives whole, in order
    Job &J = job->j;
    J.assign_units();
    std::stable_sort(fin.begin(), fin.end(), [&](const Rec &a, const Rec &b) {
        const int32_t ua = J.contigs[(size_t)a.chrom].unit, ub = J.contigs[(size_t)b.chrom].unit;
        if (ua != ub) return ua < ub;
        if (a.start != b.start) return a.start < b.start;
        return a.end < b.end;
    });
    J.postprocessed = true;
}

int bwtmi_job_import(bwtmi_job *job, const uint8_t *buf, int64_t len) {
    return guard([&] { import_wire(job, buf, len); });
}

int bwtmi_job_set_records(bwtmi_job *job, const uint8_t *buf, int64_t len) {
    return guard([&] {
        CHECK_ARG(job, "null argument");
        TEXT_JOIN(job);
        job->j.drop_results();
        import_wire(job, buf, len);
    });
}

int bwtmi_wire_record_size(void) { return (int)sizeof(WireRec); }

int64_t bwtmi_job_contig_error(const bwtmi_job *job, int32_t id, char *buf, int64_t cap) {
    if (!job || id < 0 || id >= (int32_t)job->j.contigs.size()) return -1;
    if ((size_t)id >= job->j.errors.size()) return 0;
    const std::string &e = job->j.errors[(size_t)id];
    if (buf && cap > 0) {
        const size_t m = std::min<size_t>((size_t)cap - 1, e.size());
        std::memcpy(buf, e.data(), m);
        buf[m] = 0;
    }
    return (int64_t)e.size();
}

int bwtmi_job_stage_ms(const bwtmi_job *job, double *out8) {
    return guard([&] {
        CHECK_ARG(job && out8, "null argument");
        for (int i = 0; i < 8; ++i) out8[i] = job->j.stage_ms[i];
    });
}

int bwtmi_align_region(const char *seq, int64_t seq_len, int64_t start, int64_t end, const char *tmpl,
                       int64_t tmpl_len, double frac, int64_t max_indel, int64_t min_copies, int64_t *ints8,
                       double *mismatch_rate, char *consensus, char **variations, int64_t **copy_len,
                       int64_t **copy_err) {
    int found = 0;
    int rc = guard([&] {
        CHECK_ARG((seq || seq_len == 0) && (tmpl || tmpl_len == 0) && ints8 && mismatch_rate && consensus &&
                      variations && copy_len && copy_err, "null argument");
        *variations = nullptr;
        *copy_len = *copy_err = nullptr;
        AlignSummary s;
        std::string t(tmpl ? tmpl : "", (size_t)tmpl_len);
        if (!align_repeat_region(seq, seq_len, start, end, t, min_copies, s, frac, max_indel)) return;
        found = 1;
        ints8[0] = s.copies; ints8[1] = s.motif_len; ints8[2] = s.consumed; ints8[3] = s.max_errors;
        ints8[4] = s.tot_ins; ints8[5] = s.tot_del; ints8[6] = ints8[7] = 0;
        *mismatch_rate = s.mismatch_rate;
        std::memcpy(consensus, s.consensus.data(), s.consensus.size());
        char *v = (char *)std::malloc(s.variations.size() + 1);
        std::memcpy(v, s.variations.data(), s.variations.size());
        v[s.variations.size()] = 0;
        *variations = v;
        auto *cl = (int64_t *)std::malloc(std::max<size_t>(1, s.copy_len.size()) * 8);
        auto *ce = (int64_t *)std::malloc(std::max<size_t>(1, s.copy_err.size()) * 8);
        for (size_t i = 0; i < s.copy_len.size(); ++i) { cl[i] = s.copy_len[i]; ce[i] = s.copy_err[i]; }
        *copy_len = cl;
        *copy_err = ce;
    });
    return rc ? rc : found;
}

}  // extern "C"
