// Stand-alone check of the writers' pass and of records on demand (no GPU, no
// Python): two jobs -- one contig, and a fold unit of two contigs (chr01 / CHR1)
// with different trims, whose records are built inside postprocess -- go
// through postprocess, a file write, a background file write joined later,
// the records (bwtmi_job_export on one thread, bwtmi_job_count and
// bwtmi_job_get_records on another, at once) and reset, at several
// BWTMI_RENDER_CHUNK values and thread counts.  Every text must be the text of
// one chunk, every export the export of a job nobody wrote from.  Meant for the
// sanitizer builds of the library (make -C bwt-algorithm_amd san / tsan):
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -shared-libsan tools/render_check.cpp -Iinclude \
//       -Lbwt-algorithm_amd/build-san -lbwtmi_san -Wl,-rpath,$PWD/bwt-algorithm_amd/build-san -lpthread \
//       -o /tmp/rcc && /tmp/rcc
//   (tsan: -fsanitize=thread, build-tsan, -lbwtmi_tsan; where the loader does not find the shared
//   sanitizer runtime, add -Wl,-rpath,$(dirname $(clang++ -print-file-name=libclang_rt.asan-x86_64.so)))
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "bwtmi.h"

static uint64_t g_s = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_s ^= g_s << 13;
    g_s ^= g_s >> 7;
    g_s ^= g_s << 17;
    return (uint32_t)(g_s >> 32);
}

#define OK(x)                                                                         \
    do {                                                                              \
        if ((x) != 0) {                                                               \
            std::fprintf(stderr, "%s failed: %s\n", #x, bwtmi_last_error());          \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

// maximal runs of period L with at least mc copies, primitive units only
static std::vector<bwtmi_hit> scan(const std::string &t, int maxL, int mc) {
    std::vector<bwtmi_hit> hits;
    const int64_t n = (int64_t)t.size();
    for (int L = maxL; L >= 1; --L) {
        int64_t i = 0;
        while (i + L < n) {
            if (t[(size_t)i] != t[(size_t)(i + L)]) { ++i; continue; }
            int64_t j = i;
            while (j + L < n && t[(size_t)j] == t[(size_t)(j + L)]) ++j;
            const int64_t copies = (j + L - i) / L;
            bool prim = true;
            for (int p = 1; p < L && prim; ++p)
                if (L % p == 0) {
                    bool per = true;
                    for (int q = 0; q + p < L && per; ++q) per = t[(size_t)(i + q)] == t[(size_t)(i + q + p)];
                    prim = !per;
                }
            if (copies >= mc && prim) hits.push_back(bwtmi_hit{i, i + copies * L, L, L, copies});
            i = j + 1;
        }
    }
    return hits;
}

struct Contig {
    const char *name;
    std::string seq;
    int64_t trim;
    std::vector<bwtmi_hit> hits;
};

// planted arrays between random stretches -- every fourth followed at once by
// an array of another short unit, a compound pair -- and 1 % substitutions
static Contig generate(const char *name, size_t bases, int64_t trim) {
    std::string seq;
    const char acgt[] = "ACGT";
    while (seq.size() < bases) {
        for (uint32_t k = 20 + rnd() % 200; k > 0; --k) seq += acgt[rnd() & 3];
        const int arrays = rnd() % 4 ? 1 : 2;
        for (int a = 0; a < arrays; ++a) {
            const uint32_t L = arrays == 2 ? 2 + rnd() % 2 : 1 + rnd() % (rnd() % 4 ? 6 : 30), copies = 6 + rnd() % 20;
            std::string unit;
            for (uint32_t k = 0; k < L; ++k) unit += acgt[rnd() & 3];
            for (uint32_t c = 0; c < copies; ++c) seq += unit;
        }
    }
    for (size_t i = 0; i < seq.size(); ++i)
        if (rnd() % 100 < 1) seq[i] = acgt[rnd() & 3];
    Contig c{name, seq, trim, {}};
    c.hits = scan(seq.substr((size_t)trim, seq.size() - 2 * (size_t)trim), 40, 3);
    return c;
}

static std::string slurp(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

static std::string exported(bwtmi_job *job) {
    uint8_t *buf = nullptr;
    int64_t len = 0;
    OK(bwtmi_job_export(job, &buf, &len));
    std::string s((const char *)buf, (size_t)len);
    bwtmi_free(buf);
    return s;
}

// what a C caller does: the count sizes the buffers, then the rows; as text
static std::string counted_rows(bwtmi_job *job) {
    const int64_t n = bwtmi_job_count(job);
    std::vector<int64_t> ints((size_t)n * 9 + 1);
    std::vector<double> dbls((size_t)n * 5 + 1);
    OK(bwtmi_job_get_records(job, ints.data(), dbls.data()));
    std::string s = std::to_string((long long)n);
    for (int64_t k = 0; k < n; ++k)
        s += " " + std::to_string((long long)ints[(size_t)k * 9]) + "-" + std::to_string((long long)ints[(size_t)k * 9 + 1]) + "x" +
             std::to_string(dbls[(size_t)k * 5]);
    return s;
}

struct Result {
    std::string text, file, bg_file, records, rows;
    int64_t count = 0, count_after_reset = -1;
};

static Result run(const std::vector<Contig> &contigs, int threads, int64_t chunk, bool write_first, const std::string &tmp) {
    OK(bwtmi_knob_set("RENDER_CHUNK", chunk));
    bwtmi_params p{};
    p.min_copies = 3;
    p.max_unit_len = 120;
    p.show_progress = 1;
    p.tier2 = 1;
    p.threads = threads;
    p.sa_sample = 32;
    bwtmi_job *job = nullptr;
    OK(bwtmi_job_create(&p, &job));
    for (const Contig &c : contigs) {
        int32_t id = -1;
        OK(bwtmi_job_add_contig(job, c.name, (const uint8_t *)c.seq.data(), (int64_t)c.seq.size(), c.trim, c.trim, &id));
        OK(bwtmi_job_add_hits(job, id, c.hits.data(), (int64_t)c.hits.size()));
    }
    OK(bwtmi_job_postprocess(job));
    Result r;
    r.count = bwtmi_job_count(job);
    const std::string f1 = tmp + ".sync", f2 = tmp + ".bg";
    if (write_first) OK(bwtmi_job_write(job, BWTMI_FMT_STRFINDER, f1.c_str()));
    std::thread other([&] { r.rows = counted_rows(job); });   // two readers at once
    r.records = exported(job);
    other.join();
    if (!write_first) OK(bwtmi_job_write(job, BWTMI_FMT_STRFINDER, f1.c_str()));
    char *out = nullptr;
    int64_t len = 0;
    OK(bwtmi_job_render(job, BWTMI_FMT_STRFINDER, &out, &len));
    r.text.assign(out, (size_t)len);
    bwtmi_free(out);
    OK(bwtmi_job_write_async(job, BWTMI_FMT_STRFINDER, f2.c_str()));
    OK(bwtmi_job_reset(job));   // the background write does not read the job's records
    r.count_after_reset = bwtmi_job_count(job);
    OK(bwtmi_job_write_join(job));
    r.file = slurp(f1);
    r.bg_file = slurp(f2);
    OK(bwtmi_job_free(job));
    std::remove(f1.c_str());
    std::remove(f2.c_str());
    return r;
}

static bool check(const char *what, const std::vector<Contig> &contigs, const std::string &tmp) {
    const Result want = run(contigs, 4, int64_t(1) << 40, false, tmp);
    int runs = 0;
    for (int threads : {1, 8})
        for (int64_t chunk : {int64_t(0), int64_t(1), int64_t(3), int64_t(64)})
            for (bool write_first : {false, true}) {
                const Result r = run(contigs, threads, chunk, write_first, tmp);
                if (r.text != want.text || r.file != want.text || r.bg_file != want.text || r.records != want.records ||
                    r.rows != want.rows || r.count != want.count || r.count_after_reset != 0) {
                    std::fprintf(stderr, "%s: differs (threads %d, chunk %lld, write first %d)\n", what, threads,
                                 (long long)chunk, (int)write_first);
                    return false;
                }
                ++runs;
            }
    size_t rows = 0, compound = 0;
    for (size_t i = 0; i < want.text.size(); ++i) {
        rows += want.text[i] == '\n';
        compound += want.text.compare(i, 4, "]n+[") == 0;
    }
    std::printf("render_check ok: %s, %lld records, %zu rows, %zu compound, %d runs equal\n", what, (long long)want.count,
                rows, compound, runs);
    return rows > 100 && compound > 10;
}

int main() {
    const char *dir = std::getenv("TMPDIR");
    const std::string tmp = std::string(dir && *dir ? dir : "/tmp") + "/render_check_" + std::to_string((long long)rnd());
    if (!check("one contig", {generate("chr1", 300000, 30)}, tmp)) return 1;
    if (!check("a unit of two contigs with different trims", {generate("chr01", 60000, 30), generate("CHR1", 40000, 0)}, tmp))
        return 1;
    return 0;
}
