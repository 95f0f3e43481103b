// Stand-alone check of the host post-processing (no GPU, no Python): generated
// contigs with planted arrays, substitutions and an N run, their strict hits
// found by a plain scan here, fed through bwtmi_job_add_hits and
// bwtmi_job_postprocess with BWTMI_FOLD_CUTS=0 (no cut is used: every unit is
// one segment) and =1 (the segments between verified cuts) at several
// BWTMI_FOLD_CHUNK values and thread counts; the rendered text must be the
// same.  Two jobs: one contig, and a fold unit of two contigs (chr01 / CHR1)
// with different trims.  Meant for the sanitizer builds of the library
// (make -C bwt-algorithm_amd san / tsan):
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -shared-libsan tools/fold_cuts_check.cpp -Iinclude \
//       -Lbwt-algorithm_amd/build-san -lbwtmi_san -Wl,-rpath,$PWD/bwt-algorithm_amd/build-san -o /tmp/fcc && /tmp/fcc
//   (tsan: -fsanitize=thread, build-tsan, -lbwtmi_tsan; where the loader does not find the shared
//   sanitizer runtime, add -Wl,-rpath,$(dirname $(clang++ -print-file-name=libclang_rt.asan-x86_64.so)))
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
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

// maximal runs of period L with at least mc copies, primitive units only (a
// run whose unit has a shorter period is reported at that period)
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
    int64_t trim;                  // both ends; the hits are in the trimmed frame
    std::vector<bwtmi_hit> hits;
};

// planted arrays between random stretches, 2 % substitutions, an N run past n_at
static Contig generate(const char *name, size_t bases, size_t n_at, int64_t trim) {
    std::string seq;
    const char acgt[] = "ACGT";
    while (seq.size() < bases) {
        for (uint32_t k = rnd() % 300; k > 0; --k) seq += acgt[rnd() & 3];
        const uint32_t L = 1 + rnd() % (rnd() % 4 ? 6 : 40), copies = 3 + rnd() % 30;
        std::string unit;
        for (uint32_t k = 0; k < L; ++k) unit += acgt[rnd() & 3];
        for (uint32_t c = 0; c < copies; ++c) seq += unit;
        if (seq.size() > n_at && seq.size() < n_at + 1000) seq += std::string(20000, 'N');
    }
    for (size_t i = 0; i < seq.size(); ++i)
        if (seq[i] != 'N' && rnd() % 100 < 2) seq[i] = acgt[rnd() & 3];
    Contig c{name, seq, trim, {}};
    c.hits = scan(seq.substr((size_t)trim, seq.size() - 2 * (size_t)trim), 60, 3);
    return c;
}

static std::string run(const std::vector<Contig> &contigs, int threads, int cuts, int chunk) {
    OK(bwtmi_knob_set("FOLD_CUTS", cuts));
    OK(bwtmi_knob_set("FOLD_CHUNK", chunk));
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
    char *out = nullptr;
    int64_t len = 0;
    OK(bwtmi_job_render(job, BWTMI_FMT_STRFINDER, &out, &len));
    std::string s(out, (size_t)len);
    bwtmi_free(out);
    OK(bwtmi_job_free(job));
    return s;
}

// every FOLD_CUTS x FOLD_CHUNK x threads run of the job gives the text of the first
static bool check(const char *what, const std::vector<Contig> &contigs) {
    const std::string want = run(contigs, 4, 0, 0);
    int runs = 0;
    for (int cuts : {0, 1})
        for (int threads : {1, 8})
            for (int chunk : {0, 1, 8, 64}) {
                if (run(contigs, threads, cuts, chunk) != want) {
                    std::fprintf(stderr, "%s: FOLD_CUTS=%d differs (threads %d, chunk %d)\n", what, cuts, threads, chunk);
                    return false;
                }
                ++runs;
            }
    size_t rows = 0, bases = 0, hits = 0;
    for (char c : want) rows += c == '\n';
    for (const Contig &c : contigs) {
        bases += c.seq.size();
        hits += c.hits.size();
    }
    std::printf("fold_cuts_check ok: %s, %zu bases, %zu hits, %zu rows, %d runs equal\n", what, bases, hits, rows, runs);
    return rows > 100;
}

int main() {
    if (!check("one contig", {generate("chr1", 400000, 150000, 0)})) return 1;
    if (!check("a unit of two contigs with different trims",
               {generate("chr01", 60000, 20000, 30), generate("CHR1", 40000, 1 << 30, 0)}))
        return 1;
    return 0;
}
