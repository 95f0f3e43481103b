// outfile.cpp -- the output file's writers (outfile.h).
#include "outfile.h"

#include <fcntl.h>
#include <sys/uio.h>

namespace bwtmi {

OutFd::OutFd(const char *path) : fd(::open(path, O_WRONLY | O_CREAT, 0644)) {
    if (fd < 0) fail(BWTMI_E_IO, "cannot open %s for writing", path);
}

bool pwrite_run(int fd, const char *const *p, const size_t *n, size_t cnt, size_t at) {
    constexpr size_t kIov = 1024;
    iovec v[kIov];
    size_t k = 0, skip = 0;   // next buffer, bytes of it already written
    while (k < cnt) {
        size_t m = 0;
        for (size_t j = k; j < cnt && m < kIov; ++j) {
            const size_t off = j == k ? skip : 0;
            if (n[j] <= off) continue;
            v[m].iov_base = const_cast<char *>(p[j] + off);
            v[m].iov_len = n[j] - off;
            ++m;
        }
        if (m == 0) break;
        const ssize_t w = ::pwritev(fd, v, (int)m, (off_t)at);
        if (w <= 0) return false;
        at += (size_t)w;
        size_t left = (size_t)w;   // advance (k, skip) past the bytes written
        while (k < cnt && left >= n[k] - skip) {
            left -= n[k] - skip;
            skip = 0;
            ++k;
        }
        skip += left;
    }
    return true;
}

void pwrite_parts(const char *path, bool whole, const std::vector<Text> &parts, const std::vector<size_t> &at) {
    OutFd out(path);
    std::vector<const char *> p;
    std::vector<size_t> n;
    bool good = true;
    size_t end = 0;   // end of the last part
    for (size_t k = 0; k < parts.size() && good;) {   // runs of parts that are consecutive in the file
        size_t j = k;
        end = at[k];
        p.clear();
        n.clear();
        while (j < parts.size() && at[j] == end) {
            p.push_back(parts[j].data());
            n.push_back(parts[j].size());
            end += parts[j].size();
            ++j;
        }
        good = pwrite_run(out.fd, p.data(), n.data(), p.size(), at[k]);
        k = j;
    }
    if (!good) fail(BWTMI_E_IO, "short write to %s", path);   // ~OutFd cuts a whole-file write
    if (!out.finish(whole, end)) fail(BWTMI_E_IO, "short write to %s", path);
}

}  // namespace bwtmi
