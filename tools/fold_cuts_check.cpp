// Stand-alone check of the host post-processing paths (no GPU, no Python): a
// generated contig with planted arrays, substitutions and an N run, its strict
// hits found by a plain scan here, fed through bwtmi_job_add_hits and
// bwtmi_job_postprocess with BWTMI_FOLD_CUTS=0 (the general path) and =1 (the
// one pass over cut segments) at several BWTMI_FOLD_CHUNK values and thread
// counts; the rendered text must be the same.  Meant for the sanitizer builds
// of the library (make -C bwt-algorithm_amd san / tsan):
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -shared-libsan tools/fold_cuts_check.cpp -Iinclude \
//       -Lbwt-algorithm_amd/build-san -lbwtmi_san -Wl,-rpath,$PWD/bwt-algorithm_amd/build-san -o /tmp/fcc && /tmp/fcc
//   (tsan: -fsanitize=thread, build-tsan, -lbwtmi_tsan)
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

static std::string run(const std::string &seq, const std::vector<bwtmi_hit> &hits, int threads, int cuts, int chunk) {
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
    int32_t id = -1;
    OK(bwtmi_job_add_contig(job, "chr1", (const uint8_t *)seq.data(), (int64_t)seq.size(), 0, 0, &id));
    OK(bwtmi_job_add_hits(job, id, hits.data(), (int64_t)hits.size()));
    OK(bwtmi_job_postprocess(job));
    char *out = nullptr;
    int64_t len = 0;
    OK(bwtmi_job_render(job, BWTMI_FMT_STRFINDER, &out, &len));
    std::string s(out, (size_t)len);
    bwtmi_free(out);
    OK(bwtmi_job_free(job));
    return s;
}

int main() {
    std::string seq;
    const char acgt[] = "ACGT";
    while (seq.size() < 400000) {
        for (uint32_t k = rnd() % 300; k > 0; --k) seq += acgt[rnd() & 3];
        const uint32_t L = 1 + rnd() % (rnd() % 4 ? 6 : 40), copies = 3 + rnd() % 30;
        std::string unit;
        for (uint32_t k = 0; k < L; ++k) unit += acgt[rnd() & 3];
        for (uint32_t c = 0; c < copies; ++c) seq += unit;
        if (seq.size() > 150000 && seq.size() < 151000) seq += std::string(20000, 'N');
    }
    for (size_t i = 0; i < seq.size(); ++i)
        if (seq[i] != 'N' && rnd() % 100 < 2) seq[i] = acgt[rnd() & 3];
    const std::vector<bwtmi_hit> hits = scan(seq, 60, 3);
    const std::string want = run(seq, hits, 4, 0, 0);
    int runs = 0;
    for (int threads : {1, 8})
        for (int chunk : {0, 1, 8, 64}) {
            if (run(seq, hits, threads, 1, chunk) != want) {
                std::fprintf(stderr, "FOLD_CUTS=1 differs (threads %d, chunk %d)\n", threads, chunk);
                return 1;
            }
            ++runs;
        }
    size_t rows = 0;
    for (char c : want) rows += c == '\n';
    std::printf("fold_cuts_check ok: %zu bases, %zu hits, %zu rows, %d runs equal the general path\n", seq.size(),
                hits.size(), rows, runs);
    return 0;
}
