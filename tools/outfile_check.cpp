// build: /opt/rocm/llvm/bin/clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/outfile_check.cpp bwt-algorithm_amd/csrc/outfile.cpp bwt-algorithm_amd/csrc/mem.cpp -lpthread -o /tmp/outfile_check && mkdir -p /tmp/outfile_check.d && /tmp/outfile_check /tmp/outfile_check.d
// The output-file writers (csrc/outfile.h: pwrite_parts, FileWrite) and
// lpt_assign (csrc/common.h) under ASan + UBSan, without Python or a device:
// every file is written into the directory argv[1], read back with read() and
// compared with an image built in memory.  Exit status 0 when all of it holds.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <thread>
#include <vector>

#include "../bwt-algorithm_amd/csrc/outfile.h"

namespace bwtmi {
void fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw Error{code, buf};
}
}  // namespace bwtmi

using namespace bwtmi;

static int g_bad = 0;
static void expect(bool ok, const char *what) {
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++g_bad;
}

static bool slurp(const std::string &path, std::string &out) {
    out.clear();
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) return false;
    char buf[65536];
    ssize_t r;
    while ((r = ::read(fd, buf, sizeof buf)) > 0) out.append(buf, (size_t)r);
    ::close(fd);
    return r == 0;
}

static void put(const std::string &path, const std::string &bytes) {
    const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0 || ::write(fd, bytes.data(), bytes.size()) != (ssize_t)bytes.size()) fail(BWTMI_E_IO, "cannot prepare %s", path.c_str());
    ::close(fd);
}

static bool file_is(const std::string &path, const std::string &want) {
    std::string got;
    return slurp(path, got) && got == want;
}

// part k: n bytes, none of them 0
static std::string part_bytes(size_t k, size_t n) {
    std::string s(n, 0);
    for (size_t j = 0; j < n; ++j) s[j] = (char)(1 + (k * 131 + j * 7) % 251);
    return s;
}

// nparts parts (every `empty_every`-th of them empty, 0: none) back to back from
// offset 0, with a gap of `gap` bytes after part `gap_after`; the image gets the
// parts at their offsets
static void layout(size_t nparts, size_t len, size_t gap_after, size_t gap, size_t empty_every, std::vector<Text> &parts,
                   std::vector<size_t> &at, std::string &image) {
    size_t off = 0;
    for (size_t k = 0; k < nparts; ++k) {
        const std::string s = part_bytes(k, empty_every && k % empty_every == 0 ? 0 : len);
        parts.emplace_back(s.data(), s.size());
        at.push_back(off);
        if (image.size() < off + s.size()) image.resize(off + s.size(), 0);
        image.replace(off, s.size(), s);
        off += s.size();
        if (k == gap_after) off += gap;
    }
}

static void check_pwrite_parts(const std::string &dir) {
    const std::vector<Text> none;
    const std::vector<size_t> none_at;
    {   // (a)
        const std::string p = dir + "/a.out";
        ::unlink(p.c_str());
        pwrite_parts(p.c_str(), false, none, none_at);
        struct stat st;
        expect(::stat(p.c_str(), &st) == 0 && st.st_size == 0, "(a) no parts, missing path: an empty file");
    }
    {   // (b)
        const std::string p = dir + "/b.out";
        put(p, std::string(4096, 's'));
        pwrite_parts(p.c_str(), true, none, none_at);
        expect(file_is(p, ""), "(b) no parts, whole, over a stale 4 KB file: cut to 0");
        put(p, std::string(4096, 's'));
        pwrite_parts(p.c_str(), false, none, none_at);
        expect(file_is(p, std::string(4096, 's')), "(b) no parts, not whole: the file is left alone");
    }
    for (size_t empty_every : {(size_t)0, (size_t)7}) {   // (c), (d)
        const std::string p = dir + (empty_every ? "/d.out" : "/c.out");
        std::vector<Text> parts;
        std::vector<size_t> at;
        std::string image;
        layout(3000, 37, 1500, 11, empty_every, parts, at, image);
        if (empty_every) {   // (part 0, which starts the first run, is empty) also an empty part last
            parts.emplace_back("", 0);
            at.push_back(image.size());
        }
        put(p, std::string(image.size(), 0));
        pwrite_parts(p.c_str(), false, parts, at);
        bool gap_zero = true;
        const size_t g = at[1501] - 11;
        for (size_t j = 0; j < 11; ++j) gap_zero = gap_zero && image[g + j] == 0;
        expect(gap_zero && file_is(p, image),
               empty_every ? "(d) the same with empty parts mixed in" : "(c) 3000 parts in two runs around a gap");
    }
    {   // (e)
        const std::string p = dir + "/e.out";
        std::vector<Text> parts;
        std::vector<size_t> at;
        std::string image;
        layout(40, 37, 40, 0, 0, parts, at, image);
        put(p, std::string(3 * image.size(), 's'));
        pwrite_parts(p.c_str(), true, parts, at);
        expect(image.size() == at.back() + 37 && file_is(p, image), "(e) whole: a longer stale file is cut to the last part's end");
    }
}

static void check_file_write(const std::string &dir) {
    const std::string p = dir + "/f.out";
    std::string image = "#header line\n";
    put(p, std::string(64 * 1024, 's'));
    {
        FileWrite w(p.c_str());
        w.R.header = image;
        for (size_t k = 0; k < 64; ++k) {
            const std::string s = part_bytes(k, 50 + k);
            w.R.parts.emplace_back(s.data(), s.size());
            image += s;
        }
        w.th = std::thread([&w] { w.run(); });
        auto mark = [&w](size_t first) {   // parts first, first - 2, ... done
            for (size_t k = first + 2; k >= 2; k -= 2) w.part_done(k - 2);
        };
        std::thread a(mark, 63), b(mark, 62);
        a.join();
        b.join();
        w.render_done();
        expect(w.finish() && file_is(p, image), "(f) FileWrite: 64 parts done in reverse order from two threads");
    }
    const std::string q = dir + "/f_abort.out";
    put(q, std::string(4096, 's'));
    {
        FileWrite w(q.c_str());
        w.R.header = "#header line\n";
        w.R.parts.emplace_back("row\n", 4);
        w.th = std::thread([&w] { w.run(); });
        w.part_done(0);
        w.abort();
    }
    expect(file_is(q, ""), "(f) FileWrite destroyed after abort() without finish(): a 0-byte file");
}

static void check_lpt_assign() {
    using V = std::vector<size_t>;
    expect(lpt_assign({10, 40, 30, 20}, 2) == V{0, 0, 1, 1}, "(g) {10,40,30,20} over 2 bins");
    expect(lpt_assign({5, 5, 5, 5, 5, 5, 5}, 3) == V{0, 1, 2, 0, 1, 2, 0}, "(g) equal weights: round-robin from bin 0");
    expect(lpt_assign({3, 9}, 5) == V{1, 0}, "(g) more bins than items: the high bins stay empty");
    expect(lpt_assign({}, 4).empty(), "(g) no items");
    expect(lpt_assign({7, 7, 2, 2, 9}, 2) == V{1, 1, 0, 0, 0}, "(g) ties keep item order, the lighter bin is next");
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s DIRECTORY\n", argv[0]);
        return 2;
    }
    try {
        check_pwrite_parts(argv[1]);
        check_file_write(argv[1]);
        check_lpt_assign();
    } catch (const Error &e) {
        std::printf("FAIL error %d: %s\n", e.code, e.msg.c_str());
        return 1;
    }
    std::printf("%d failed\n", g_bad);
    return g_bad != 0;
}
