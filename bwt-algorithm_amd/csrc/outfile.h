// outfile.h -- writing the output file: POSIX host code only (no HIP), so it
// links into a stand-alone program (tools/outfile_check.cpp).
#pragma once

#include <unistd.h>

#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "common.h"

namespace bwtmi {

// Output file descriptor: closed on every path; when the write fails part-way
// (an exception or a short write) the file is cut to 0 bytes rather than left
// holding a mix of old and new rows.
struct OutFd {
    int fd = -1;
    bool ok = false;
    explicit OutFd(const char *path);   // opens (and creates) path; fails with BWTMI_E_IO
    ~OutFd() {
        if (fd < 0) return;
        [[maybe_unused]] const int cut = ok ? 0 : ::ftruncate(fd, 0);
        (void)::close(fd);
    }
    // cut to `size` (when whole) and close; false on error
    bool finish(bool whole, size_t size) {
        bool good = !whole || ::ftruncate(fd, (off_t)size) == 0;
        ok = good;
        good = (::close(fd) == 0) && good;
        fd = -1;
        return good;
    }
};

// Buffers [p[k], p[k] + n[k]) written back to back at byte offset `at` of fd,
// IOV_MAX at a time: one writer with large pwritev calls.  Buffered writes to
// one file serialise on its inode lock, so parallel writers only contend: on
// the box host a 55 MB file took 2.8-3.1 ms as one pwrite and 4.3-4.8 ms from
// 16 threads (tools/write_bench.cpp, profiles/r06/write_bench_r06g.txt).
// False on a short write.
bool pwrite_run(int fd, const char *const *p, const size_t *n, size_t cnt, size_t at);

// parts[k] lands at byte offset at[k] of `path` (one writer, consecutive parts
// in one pwritev).  `whole`: the parts are the whole file -- it is overwritten
// in place and cut to the end of its last part afterwards (the content is that
// of open(path, 'w') + write; rewriting a file of the same size reuses its
// page-cache pages).  No parts: the file is opened (and created) and closed,
// cut to 0 bytes when `whole`.
void pwrite_parts(const char *path, bool whole, const std::vector<Text> &parts, const std::vector<size_t> &at);

// One output file written by its own writer thread while the rows are being
// formatted (bwtmi_job_write, bwtmi_job_write_async).  The formatting tasks
// mark their part done; the writer pwritev's every run of consecutive done
// parts in file order, the header first -- ONE writer, since buffered writes
// to one file serialise on its inode lock (pwrite_run).  The content is that
// of one open(path, 'w') + write: the file is overwritten in place and cut to
// its size at the end (a short write or an error cuts it to 0).
struct FileWrite {
    OutFd out;
    std::string path;
    Rendered R;
    std::mutex mu;
    std::condition_variable cv;
    std::vector<uint8_t> done;
    size_t next = 0, off = 0;
    bool started = false, rendered = false, aborted = false, header_done = false, bad = false;
    std::thread th;
    explicit FileWrite(const char *p) : out(p), path(p) {}
    ~FileWrite() {
        if (th.joinable()) {
            abort();
            th.join();
        }
    }
    void part_done(size_t k) {   // (render_rows sized R.parts before the first part)
        {
            std::lock_guard<std::mutex> lk(mu);
            if (!started) {
                done.assign(R.parts.size(), 0);
                started = true;
            }
            done[k] = 1;
        }
        cv.notify_one();
    }
    void render_done() {
        {
            std::lock_guard<std::mutex> lk(mu);
            rendered = true;
        }
        cv.notify_one();
    }
    void abort() {
        {
            std::lock_guard<std::mutex> lk(mu);
            rendered = aborted = true;
        }
        cv.notify_one();
    }
    void run() {   // the writer thread's body
        std::unique_lock<std::mutex> lk(mu);
        std::vector<const char *> wp;
        std::vector<size_t> wn;
        auto ready = [&] { return started && next < done.size() && done[next]; };
        for (;;) {
            cv.wait(lk, [&] { return aborted || rendered || (started && !header_done) || ready(); });
            if (aborted) return;
            if (!header_done) {   // the header exists once a part or the whole render is done
                header_done = true;
                const char *hp = R.header.data();
                const size_t hn = R.header.size();
                off = hn;
                lk.unlock();
                if (!pwrite_run(out.fd, &hp, &hn, 1, 0)) bad = true;
                lk.lock();
                continue;
            }
            if (ready()) {
                const size_t at = off;
                wp.clear();
                wn.clear();
                while (ready()) {
                    wp.push_back(R.parts[next].data());
                    wn.push_back(R.parts[next].size());
                    off += R.parts[next].size();
                    ++next;
                }
                lk.unlock();
                if (!pwrite_run(out.fd, wp.data(), wn.data(), wp.size(), at)) bad = true;
                lk.lock();
                continue;
            }
            if (rendered) return;   // every part is done and written
        }
    }
    // wait for the writer, cut the file to its size and close it; false on a short write
    bool finish() {
        if (th.joinable()) th.join();
        return !bad && !aborted && out.finish(true, off);
    }
};

}  // namespace bwtmi
