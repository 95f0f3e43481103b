// render.cpp -- compound detection and the five output writers
// (TandemRepeatFinder.save_results bwt.py:4141-4198, _detect_compound_repeats
// 3995-4139, _simple_kmer_scan 3956-3993, TandemRepeat.to_* 454-641).
// Python's "{x:.Nf}" and C's "%.Nf" both print the exact binary value rounded
// half-to-even, so numeric columns are byte-identical.
#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <thread>
#include <optional>
#include <chrono>
#include <cinttypes>
#include <cmath>
#include <charconv>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "common.h"
#include "fmtnum.h"

namespace bwtmi {
namespace {

struct View {
    const char *p = nullptr;
    int64_t n = 0;
    bool empty() const { return n <= 0; }
};

// the view of a final record (valid while the record and its contig's text are)
RecRef ref_of(const Job &job, const Rec &r) {
    RecRef v;
    v.start = r.start;
    v.end = r.end;
    v.copies = r.copies;
    v.pmatch = r.pmatch;
    v.pindel = r.pindel;
    v.mismatch_rate = r.mismatch_rate;
    v.confidence = r.confidence;
    v.n_eval = r.n_eval;
    v.max_mm = r.max_mm;
    v.score = r.score;
    v.motif = r.motif.data();
    v.mlen = (int32_t)r.motif.size();
    v.var = r.variations.data();
    v.vlen = (int32_t)r.variations.size();
    if (r.act_kind != ACT_NONE) {
        const Contig &c = job.contigs[(size_t)r.chrom];
        v.act = (r.act_kind == ACT_FULL ? c.full.data() : c.trimmed()) + r.act_off;
        v.act_len = r.act_len;
    }
    v.chrom = r.chrom;
    v.tier = r.tier;
    v.strand = r.strand;
    v.kmer_stats = r.kmer_stats;
    v.stats_none = r.stats_none;
    return v;
}

// a compound-stage piece (bwt.py:3980-3987, 4074-4091): its motif and its
// actual sequence are bytes of the contig
RecRef piece_ref(int32_t chrom, int64_t start, int64_t end, const char *motif, int32_t mlen, int64_t copies,
                 int32_t tier, const char *act, int64_t act_len) {
    RecRef v;
    v.start = start;
    v.end = end;
    v.copies = (double)copies;
    v.pmatch = 100.0;
    v.pindel = 0.0;
    v.mismatch_rate = 0.0;
    v.confidence = 1.0;
    v.n_eval = copies;
    v.max_mm = 0;
    v.score = 100;
    v.motif = motif;
    v.mlen = mlen;
    v.act = act;
    v.act_len = act_len;
    v.chrom = chrom;
    v.tier = tier;
    v.strand = '+';
    v.kmer_stats = true;
    return v;
}

inline bool same_motif(const RecRef &a, const RecRef &b) {
    return a.mlen == b.mlen && std::memcmp(a.motif, b.motif, (size_t)a.mlen) == 0;
}

// _simple_kmer_scan(chrom, start, end, k=3, use_full_seq=True)
void kmer_scan(const Job &job, int32_t chrom, int64_t start, int64_t end, std::vector<RecRef> &out) {
    const Seq &seq = job.contigs[(size_t)chrom].full;
    const int64_t L = (int64_t)seq.size();
    const int64_t k = 3;
    if (seq.empty() || start >= end || start < 0 || end > L) return;
    const char *reg = seq.data() + start;
    const int64_t rl = end - start;
    int64_t i = 0;
    while (i < rl - k) {
        int64_t c = 1, j = i + k;
        while (j + k <= rl && std::memcmp(reg + j, reg + i, (size_t)k) == 0) {
            ++c;
            j += k;
        }
        if (c >= 5) {
            out.push_back(piece_ref(chrom, start + i, start + j, reg + i, (int32_t)k, c, 1, reg + i, j - i));
            i = j;
        } else {
            ++i;
        }
    }
}

// span of a > 10 bp motif, with the prefix maximum of the ends up to it
struct Long { int64_t s, e, pe; };

// The records one walk of _detect_compound_repeats (bwt.py:3995-4139) runs
// over: one chromosome's final records in start order with the k-mer pieces
// merged in behind the records of equal start (the reference appends them and
// sorts stably by start, bwt.py:4011-4026).  The merged list is never built:
// index m is piece k when ppos[k] == m, else final record m - (pieces before m).
struct Merged {
    const Rec *main = nullptr;          // n_main consecutive records, or
    const Rec *const *list = nullptr;   // n_main pointers, or
    const Survivors *sv = nullptr;      // the fold's survivors of unit su
    size_t su = 0;
    size_t n_main = 0;
    const RecRef *pieces = nullptr;
    const size_t *ppos = nullptr;
    size_t np = 0;
    const Long *longs = nullptr;
    size_t nl = 0;
    int32_t chrom = 0;
    size_t size() const { return n_main + np; }
    const Rec &rec(size_t k) const { return list ? *list[k] : main[k]; }
    // m is a piece: its index (true); else the final record's index
    bool piece_at(size_t m, size_t &k) const {
        k = m;
        if (!np) return false;
        const size_t q = (size_t)(std::lower_bound(ppos, ppos + np, m) - ppos);
        if (q < np && ppos[q] == m) {
            k = q;
            return true;
        }
        k = m - q;
        return false;
    }
    int64_t main_start(size_t k) const {
        if (!sv) return rec(k).start;
        int64_t s, e;
        int32_t ml;
        sv->span(su, k, s, e, ml);
        return s;
    }
    // final records with a start <= s
    size_t mains_upto(int64_t s) const {
        size_t lo = 0, hi = n_main;
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            if (s < main_start(mid)) hi = mid;
            else lo = mid + 1;
        }
        return lo;
    }
    RecRef view(const Job &job, size_t m) const {
        size_t k;
        return piece_at(m, k) ? pieces[k] : sv ? sv->view(su, k) : ref_of(job, rec(k));
    }
    int64_t start_at(size_t m) const {
        size_t k;
        return piece_at(m, k) ? pieces[k].start : main_start(k);
    }
};

// one row of a walk: indices into the walk's views (>= 0) or its split pieces (~index)
struct WRow { int32_t r, p; };
constexpr int32_t kNoRec = INT32_MIN;
// a row ready for the formatter (bwt.py:4126-4130: a record or a compound
// piece, with its partner)
struct FRow { const RecRef *r, *p; };

// A walk from merged index m0.  Its only state is the index; a step consumes 1
// or 2 records, or more after splits, and emits rows.  The views are built as
// the walk reaches them; rows hold indices and are resolved to pointers once
// the walk is over (the vectors may grow until then).
struct Walk {
    const Job &job;
    const Merged &M;
    const size_t m0;
    std::vector<RecRef> vw, spl;
    std::vector<WRow> rows;
    std::vector<uint32_t> at;   // rows[k] was emitted by the step from m0 + at[k]
    std::vector<int32_t> run_from;
    Walk(const Job &j, const Merged &m, size_t from, size_t expect = 0) : job(j), M(m), m0(from) {
        vw.reserve(expect + 8);
        rows.reserve(expect + 8);
        at.reserve(expect + 8);
    }
    void reach(size_t m) {   // views up to m exist (earlier references may move)
        while (vw.size() <= m - m0) vw.push_back(M.view(job, m0 + vw.size()));
    }
    const RecRef *ref(int32_t x) const { return x == kNoRec ? nullptr : x >= 0 ? &vw[(size_t)x] : &spl[(size_t)~x]; }
    void emit(int32_t r, int32_t p, size_t i0) {
        rows.push_back({r, p});
        at.push_back((uint32_t)(i0 - m0));
    }
    void plain(size_t i) {   // the formats without compounds: every record is a row
        reach(i);
        emit((int32_t)(i - m0), kNoRec, i);
    }
    size_t step(size_t i) {
        const size_t i0 = i, N = M.size();
        reach(std::min(i + 1, N - 1));
        const RecRef cur = vw[i - m0];   // (a copy: the views may move below)
        const Contig &ctg = job.contigs[(size_t)M.chrom];
        const int64_t TL = ctg.trimmed_len();
        if (cur.mlen == 3 && cur.copies >= 10 && TL > 0) {
            // repeat_seq = sequences[chrom][cur.start:cur.end] (trimmed sequence, restored
            // coordinates -- bwt.py:4045-4047)
            const char *tseq = ctg.trimmed();
            const int64_t a = std::min(std::max<int64_t>(cur.start, 0), TL);
            const int64_t b = std::max(a, std::min(std::max<int64_t>(cur.end, 0), TL));
            const char *rsq = tseq + a;
            const int64_t rl = b - a;
            const int64_t k = 3;
            // Every split point sp (k <= sp < rl - k, a multiple of k) sees whole
            // copies only: l1 = l2 = k, c1 = the leading copies equal to copy 0,
            // capped at sp / k, and c2 = the run of copies equal to copy sp/k
            // (exact equality chains), so both come from one pass over the
            // copies instead of a rescan per split point (O(copies), not O(copies^2))
            const int64_t nq = rl / k;   // whole copies
            int64_t lead = 0;
            if (rl - k > k) {
                while (lead < nq && std::memcmp(rsq + lead * k, rsq, (size_t)k) == 0) ++lead;
                run_from.assign((size_t)nq + 1, 0);
                for (int64_t q = nq - 1; q >= 0; --q)
                    run_from[(size_t)q] = 1 + (q + 1 < nq && std::memcmp(rsq + q * k, rsq + (q + 1) * k, (size_t)k) == 0
                                                   ? run_from[(size_t)q + 1] : 0);
            }
            for (int64_t sp = k; sp < rl - k; sp += k) {
                const int64_t l1 = k, l2 = k;
                if (std::memcmp(rsq, rsq + sp, (size_t)k) == 0) continue;
                const int64_t c1 = std::min<int64_t>(lead, sp / k);
                const int64_t c2 = run_from[(size_t)(sp / k)];
                if (c1 >= 5 && c2 >= 5 && (double)(c1 * l1 + c2 * l2) >= (double)rl * 0.9) {
                    const int64_t e1 = cur.start + c1 * l1;
                    // actual = repeat_seq[:c1*l1], repeat_seq[c1*l1 : c1*l1 + c2*l2]
                    const int64_t x1 = std::min(c1 * l1, rl);
                    const int64_t y0 = std::min(c1 * l1, rl), y1 = std::max(y0, std::min(c1 * l1 + c2 * l2, rl));
                    spl.push_back(piece_ref(M.chrom, cur.start, e1, rsq, (int32_t)l1, c1, cur.tier, tseq + a, x1));
                    spl.push_back(piece_ref(M.chrom, e1, e1 + c2 * l2, rsq + sp, (int32_t)l2, c2, cur.tier,
                                            tseq + a + y0, y1 - y0));
                    emit(~(int32_t)(spl.size() - 2), ~(int32_t)(spl.size() - 1), i0);
                    ++i;   // the reference advances i inside the split loop (bwt.py:4083)
                }
            }
        }
        if (i + 1 < N) {
            reach(i + 1);
            const RecRef &nx = vw[i + 1 - m0];
            const int64_t gap = nx.start - cur.end;
            if (gap <= 5 && cur.mlen <= 4 && nx.mlen <= 4 && !same_motif(cur, nx) && cur.copies >= 5 && nx.copies >= 5) {
                const int64_t cs = cur.start, ce = nx.end;
                // any(long overlaps >= 80 %): a long with s >= ce or e <= cs has
                // ov = 0, so only those before the first s >= ce whose prefix
                // max end still exceeds cs can qualify
                bool covered = false;
                size_t k = (size_t)(std::lower_bound(M.longs, M.longs + M.nl, ce,
                                                     [](const Long &l, int64_t x) { return l.s < x; }) - M.longs);
                while (k > 0 && !covered) {
                    const Long &lm = M.longs[--k];
                    if (lm.pe <= cs) break;
                    const int64_t ov = std::max<int64_t>(0, std::min(ce, lm.e) - std::max(cs, lm.s));
                    if ((double)ov / (double)(ce - cs) >= 0.8) covered = true;
                }
                if (!covered) {
                    emit((int32_t)(i0 - m0), (int32_t)(i + 1 - m0), i0);
                    return i + 2;
                }
            }
        }
        emit((int32_t)(i0 - m0), kNoRec, i0);
        return i + 1;
    }
    void resolve(std::vector<FRow> &out) const {
        for (const WRow &w : rows) out.push_back({ref(w.r), ref(w.p)});
    }
};

// rows in start order: the runs of equal start go by end, stably -- which makes
// them sorted(key=(start, end)) (bwt.py:4150; runs are short)
void order_equal_starts(std::vector<FRow> &rows) {
    for (size_t i = 0; i < rows.size();) {
        size_t j = i + 1;
        while (j < rows.size() && rows[j].r->start == rows[i].r->start) ++j;
        for (size_t a = i + 1; a < j; ++a) {
            const FRow x = rows[a];
            size_t q = a;
            while (q > i && rows[q - 1].r->end > x.r->end) {
                rows[q] = rows[q - 1];
                --q;
            }
            rows[q] = x;
        }
        i = j;
    }
}

// ---------------------------------------------------------------- formatting
struct Out {
    // rows are written through a raw cursor into s (sized ahead, grown by
    // doubling); finish() cuts s to what was written
    Text s;
    char *w = nullptr, *e = nullptr;
    std::string built, core;   // per-chunk scratch of the row formatters (no thread-local lookups per row)
    size_t used() const { return w ? (size_t)(w - s.data()) : 0; }
    void reserve(size_t n) {
        const size_t u = used();
        s.set_size(u);
        s.grow(u + n);
        w = s.data() + u;
        e = s.data() + s.capacity();
    }
    void need(size_t n) {
        if ((size_t)(e - w) < n) reserve(std::max(n, s.capacity()));
    }
    Text finish() {
        s.set_size(used());
        w = e = nullptr;
        return std::move(s);
    }
    void put(const char *p, int64_t n) {
        if (n <= 0) return;
        need((size_t)n);
        std::memcpy(w, p, (size_t)n);
        w += n;
    }
    void put(const std::string &x) { put(x.data(), (int64_t)x.size()); }
    void put(View v) { put(v.p, v.n); }
    void c(char ch) {
        need(1);
        *w++ = ch;
    }
    void f(const char *fmt, double x) {   // printf keeps Python's exact-value rounding
        if (fmt[1] == '.' && fmt[2] == '0' && fmt[3] == 'f' && std::fabs(x) < 1e15 && !std::signbit(x)) {
            // %.0f rounds the exact binary value to nearest, ties to even --
            // nearbyint in the default rounding mode, without printf
            i((int64_t)std::nearbyint(x));
            return;
        }
        if (fmt[1] == '.' && fmt[2] >= '1' && fmt[2] <= '3' && fmt[3] == 'f') {   // exact, no printf (fmtnum.h)
            need(40);
            if (char *end = fixed_dec(x, fmt[2] - '0', w)) {
                w = end;
                return;
            }
        }
        char b[64];
        int n = snprintf(b, sizeof b, fmt, x);
        put(b, n);
    }
    void i(int64_t x) {   // decimal (std::to_chars took a third of the rows' time)
        need(24);
        w = int_dec(x, w);
    }
    void rep(const char *m, int64_t len, int64_t times) {
        for (int64_t k = 0; k < times; ++k) put(m, len);
    }
};

inline int64_t py_round(double x) { return (int64_t)std::nearbyint(x); }

void comp_entropy(const RecRef &r, double comp[4], double &ent) {
    if (r.kmer_stats) {
        comp[0] = comp[1] = comp[2] = comp[3] = 0.0;
        ent = 1.5;
        return;
    }
    if (r.stats_none) {   // to_trf_table/to_trf_dat: composition or 25 % each (bwt.py:485, 505)
        comp[0] = comp[1] = comp[2] = comp[3] = 25.0;
        ent = 0.0;
        return;
    }
    composition_of(r.motif, r.mlen, comp);
    ent = entropy_of(r.motif, r.mlen);
}

void row_strfinder(Out &o, const Job &job, const RecRef &r, const RecRef *partner) {
    const Contig &c = job.contigs[(size_t)r.chrom];
    const Seq &full = c.full;
    const int64_t FL = (int64_t)full.size();
    View fl, fr;
    if (!full.empty()) {   // full[max(0,start-30):start], full[end:end+30]
        int64_t a = std::min(std::max<int64_t>(0, r.start - 30), FL), b = std::min(std::max<int64_t>(r.start, 0), FL);
        if (b > a) { fl.p = full.data() + a; fl.n = b - a; }
        a = std::min(std::max<int64_t>(r.end, 0), FL);
        b = std::min(std::max<int64_t>(r.end + 30, 0), FL);
        if (b > a) { fr.p = full.data() + a; fr.n = b - a; }
    }
    const bool flanks = !fl.empty() || !fr.empty();
    o.put("STR_");
    o.put(c.name);
    o.c('\t');
    if (partner) {
        const RecRef &p = *partner;
        const int64_t k1 = py_round(r.copies), k2 = py_round(p.copies);
        std::string &core = o.core;
        core.clear();
        if (r.act_len > 0) core.append(r.act, (size_t)r.act_len);
        else for (int64_t k = 0; k < k1; ++k) core.append(r.motif, (size_t)r.mlen);
        if (p.act_len > 0) core.append(p.act, (size_t)p.act_len);
        else for (int64_t k = 0; k < k2; ++k) core.append(p.motif, (size_t)p.mlen);
        o.put(c.name); o.c(':'); o.i(r.start + 1); o.c('-'); o.i(p.end); o.c('\t');
        o.c('['); o.put(r.motif, r.mlen); o.put("]n+["); o.put(p.motif, p.mlen); o.put("]n\t");
        o.i(r.mlen); o.c('['); o.put(r.motif, r.mlen); o.c(']'); o.i(k1); o.c(';');
        o.i(p.mlen); o.c('['); o.put(p.motif, p.mlen); o.c(']'); o.i(k2); o.put(",0\t");
        o.i(k1); o.c('/'); o.i(k2); o.c('\t');
        o.put(core); o.put("\t100%\t-\t");
        o.i(k1); o.c(':'); o.i(k2); o.c('\t'); o.i(k1 + k2); o.c('\t');
        if (flanks) { o.put(fl); o.put(core); o.put(fr); } else o.put(core);
        o.put("\t-\n");
        return;
    }
    const int64_t ml = r.mlen;
    const int64_t cc = (int64_t)std::floor(r.copies + 1e-6);
    o.put(c.name); o.c(':'); o.i(r.start + 1); o.c('-'); o.i(r.end); o.c('\t');
    o.c('['); o.put(r.motif, ml); o.put("]n\t");
    o.i(ml); o.c('['); o.put(r.motif, ml); o.c(']'); o.i(cc); o.c(','); o.i((r.end - r.start) - ml * cc); o.c('\t');
    if (std::fabs(r.copies - std::nearbyint(r.copies)) < 1e-6) {
        o.i(py_round(r.copies));
    } else {
        char b[64];
        char *e = fixed_dec(r.copies, 2, b);
        const int n = e ? (int)(e - b) : snprintf(b, sizeof b, "%.2f", r.copies);
        int m = n;
        while (m > 0 && b[m - 1] == '0') --m;
        while (m > 0 && b[m - 1] == '.') --m;
        o.put(b, m);
    }
    o.c('\t');
    // core sequence: the actual-sequence slice, or the motif repeated int(copies) times
    std::string &built = o.built;
    View core{r.act, r.act_len};
    if (core.empty()) {
        built.clear();
        for (int64_t k = 0; k < (int64_t)r.copies; ++k) built.append(r.motif, (size_t)ml);
        core.p = built.data();
        core.n = (int64_t)built.size();
    }
    if (core.n > 150) {
        o.put(core.p, 70);
        o.put("... (x"); o.i(cc); o.c(')');
    } else {
        o.put(core);
    }
    o.c('\t');
    o.f("%.0f", r.pmatch);
    o.put("%\t-\t");
    o.i(cc); o.c(':'); o.i(r.n_eval); o.c('\t'); o.i(r.n_eval); o.c('\t');
    const int64_t tot = (flanks ? fl.n + fr.n : 0) + core.n;
    if (tot > 500) {   // full_seq[:250] + "..." + full_seq[-200:] of fl + core + fr, without building it
        const View parts[3] = {flanks ? fl : View{}, core, flanks ? fr : View{}};
        auto put_range = [&](int64_t a, int64_t b) {   // bytes [a, b) of the concatenation
            int64_t base = 0;
            for (const View &v : parts) {
                const int64_t lo = std::max(a, base), hi = std::min(b, base + v.n);
                if (hi > lo) o.put(v.p + (lo - base), hi - lo);
                base += v.n;
            }
        };
        put_range(0, 250);
        o.put("...");
        put_range(tot - 200, tot);
    } else {
        if (flanks) { o.put(fl); o.put(core); o.put(fr); } else o.put(core);
    }
    o.c('\t');
    if (r.vlen > 0) o.put(r.var, r.vlen); else o.c('-');
    o.c('\n');
}

// one row of any format; row_id is the VCF record id
void format_row(Out &o, const Job &job, int fmt, const RecRef &r, const RecRef *partner, int64_t row_id) {
    double cp[4], ent;
    const std::string &name = job.contigs[(size_t)r.chrom].name;
    const int64_t ml = r.mlen;
    switch (fmt) {
        case BWTMI_FMT_BED:
            o.put(name); o.c('\t'); o.i(r.start); o.c('\t'); o.i(r.end);
            o.c('\t'); o.put(r.motif, ml); o.c('\t'); o.f("%.1f", r.copies); o.c('\t'); o.i(r.tier); o.c('\t');
            o.f("%.3f", r.mismatch_rate); o.c('\t'); o.c(r.strand); o.c('\n');
            break;
        case BWTMI_FMT_VCF:
            o.put(name); o.c('\t'); o.i(r.start + 1); o.put("\tTR"); o.i(row_id);
            o.put("\t.\t<TR>\t.\tPASS\tMOTIF="); o.put(r.motif, ml); o.put(";CONS_MOTIF="); o.put(r.motif, ml);
            o.put(";COPIES="); o.f("%.1f", r.copies); o.put(";TIER="); o.i(r.tier);
            o.put(";CONF="); o.f("%.2f", r.confidence); o.put(";MM_RATE="); o.f("%.3f", r.mismatch_rate);
            o.put(";MAX_MM_PER_COPY="); o.i(r.max_mm); o.put(";N_COPIES_EVAL="); o.i(r.n_eval);
            o.put(";STRAND="); o.c(r.strand); o.c('\n');
            break;
        case BWTMI_FMT_TRF_TABLE:
            comp_entropy(r, cp, ent);
            o.i(r.start); o.put("--"); o.i(r.end); o.c('\t'); o.i(ml); o.c('\t'); o.f("%.1f", r.copies);
            o.c('\t'); o.i(ml); o.c('\t'); o.f("%.0f", r.pmatch); o.c('\t'); o.f("%.0f", r.pindel); o.c('\t');
            o.i(r.score); o.c('\t'); o.f("%.0f", cp[0]); o.c('\t'); o.f("%.0f", cp[1]); o.c('\t');
            o.f("%.0f", cp[2]); o.c('\t'); o.f("%.0f", cp[3]); o.c('\t'); o.f("%.2f", ent); o.c('\n');
            break;
        case BWTMI_FMT_TRF_DAT:
            comp_entropy(r, cp, ent);
            o.i(r.start); o.c(' '); o.i(r.end); o.c(' '); o.i(ml); o.c(' '); o.f("%.1f", r.copies); o.c(' ');
            o.i(ml); o.c(' '); o.f("%.0f", r.pmatch); o.c(' '); o.f("%.0f", r.pindel); o.c(' ');
            o.i(r.score); o.c(' '); o.f("%.0f", cp[0]); o.c(' '); o.f("%.0f", cp[1]); o.c(' ');
            o.f("%.0f", cp[2]); o.c(' '); o.f("%.0f", cp[3]); o.c(' '); o.f("%.2f", ent); o.c(' ');
            o.put(r.motif, ml); o.c(' ');
            if (r.act_len > 0) o.put(r.act, r.act_len); else o.rep(r.motif, ml, (int64_t)r.copies);
            o.c('\n');
            break;
        default:   // STRfinder
            row_strfinder(o, job, r, partner);
    }
}

// rows (ordered) appended to o; off (may be null) receives the byte offset of
// every row and of the end
void format_rows(Out &o, const Job &job, int fmt, const std::vector<FRow> &rows, int64_t id0, std::vector<size_t> *off) {
    // a row's flanks and core are bytes of its contig at random distances
    // from the last row's: their lines are requested a few rows ahead
    constexpr size_t kAhead = 6;
    auto prefetch_row = [&](const RecRef &r) {
        const Seq &full = job.contigs[(size_t)r.chrom].full;
        if (full.empty()) return;
        const int64_t FL = (int64_t)full.size();
        const int64_t s0 = std::min(std::max<int64_t>(0, r.start - 30), FL - 1), e0 = std::min(std::max<int64_t>(0, r.end), FL - 1);
        __builtin_prefetch(full.data() + s0);
        __builtin_prefetch(full.data() + s0 + 64);
        __builtin_prefetch(full.data() + e0);
    };
    const bool str = fmt == BWTMI_FMT_STRFINDER;
    const size_t n = rows.size();
    o.reserve(n * 256);
    if (off) off->reserve(off->size() + n + 1);
    if (str)
        for (size_t k = 0; k < std::min(n, kAhead); ++k) prefetch_row(*rows[k].r);
    for (size_t k = 0; k < n; ++k) {
        if (str && k + kAhead < n) prefetch_row(*rows[k + kAhead].r);
        if (off) off->push_back(o.used());
        format_row(o, job, fmt, *rows[k].r, rows[k].p, id0 + (int64_t)k);
    }
    if (off) off->push_back(o.used());
}

const char *kVcfHeader =
    "##fileformat=VCFv4.2\n"
    "##INFO=<ID=MOTIF,Number=1,Type=String,Description=\"Original seed motif\">\n"
    "##INFO=<ID=CONS_MOTIF,Number=1,Type=String,Description=\"Consensus motif from all copies\">\n"
    "##INFO=<ID=COPIES,Number=1,Type=Float,Description=\"Number of copies\">\n"
    "##INFO=<ID=TIER,Number=1,Type=Integer,Description=\"Detection tier (1=short, 2=medium/long, 3=very long)\">\n"
    "##INFO=<ID=CONF,Number=1,Type=Float,Description=\"Confidence score\">\n"
    "##INFO=<ID=MM_RATE,Number=1,Type=Float,Description=\"Overall mismatch rate across all copies\">\n"
    "##INFO=<ID=MAX_MM_PER_COPY,Number=1,Type=Integer,Description=\"Maximum mismatches in any single copy\">\n"
    "##INFO=<ID=N_COPIES_EVAL,Number=1,Type=Integer,Description=\"Number of copies evaluated for consensus\">\n"
    "##INFO=<ID=STRAND,Number=1,Type=String,Description=\"Strand of canonical motif (+/-)\">\n"
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";

// the records of one fold unit that has any, and what the pre-pass found for them
struct UnitPlan {
    int32_t unit = 0;
    // one chromosome, consecutive in the job's records, in start order: walked
    // and formatted in parallel chunks.  Anything else (records handed in in
    // another order, a unit of several chromosomes) is one chunk on one thread.
    bool regular = true;
    size_t n = 0;                        // regular: its records
    std::vector<const Rec *> list;       // not regular: the unit's records in the job's order
    std::vector<std::pair<size_t, RecRef>> found;   // k-mer pieces with the index of the record they follow
    std::vector<RecRef> pieces;          // regular: the same by start, and where they go
    std::vector<size_t> ppos;
    std::vector<Long> longs;
    int64_t base = 0;                    // VCF id of the unit's first row
    Merged M;
};

}  // namespace

// Records to bytes in one pass.  A pre-pass over the records finds the fold
// units' runs, the k-mer pieces behind 3-mer records and the > 10 bp motifs.
// Then chunks of consecutive records of one unit are walked for compounds as if
// the walk arrived at their first index, ordered and formatted, each into its
// own part, while they are in cache.  Chunk edges lie where the start grows, so
// no run of equal starts spans two chunks.  The chunks are committed in order:
// when the true walk enters a chunk elsewhere than at its first index (a step
// of the chunk before consumed records of this one), it is walked again from
// there until both walks step from the same index at the beginning of a run of
// equal starts -- from then on they are the same walk -- and only the rows up
// to there are formatted again; the bytes behind them are kept.
void render_rows(Job &job, int fmt, const int64_t *row_base, Rendered &out,
                 const std::function<void(size_t)> *on_part) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    job.assign_units();
    std::string head;
    switch (fmt) {
        case BWTMI_FMT_BED:
            head = "# Tandem Repeats (BED format with imperfect repeat support)\n"
                   "# chrom\tstart\tend\tconsensus_motif\tcopies\ttier\tmismatch_rate\tstrand\n";
            break;
        case BWTMI_FMT_VCF: head = kVcfHeader; break;
        case BWTMI_FMT_TRF_TABLE:
            head = "# Tandem Repeats Finder Compatible Table Format\n"
                   "# Indices\tPeriod\tCopyNumber\tConsensusSize\tPercentMatches\tPercentIndels\t"
                   "Score\tA\tC\tG\tT\tEntropy\n";
            break;
        case BWTMI_FMT_TRF_DAT: break;
        case BWTMI_FMT_STRFINDER:
            head = "STR_marker\tSTR_position\tSTR_motif\tSTR_genotype_structure\tSTR_genotype\t"
                   "STR_core_seq\tAllele_coverage\tAlleles_ratio\tReads_Distribution(consensused)\t"
                   "STR_depth\tFull_seq\tVariations\n";
            break;
        default:
            fail(BWTMI_E_ARG, "unknown output format %d", fmt);
    }
    const bool str = fmt == BWTMI_FMT_STRFINDER;
    const int nt = host_threads(job.params);
    auto unit_of = [&](const Rec &r) { return job.contigs[(size_t)r.chrom].unit; };
    // the k-mer pieces behind a 3-mer record ending at `end` (bwt.py:4011-4024)
    auto pieces_behind = [&](int32_t chrom, int64_t end, const char *motif, size_t q, std::vector<RecRef> &kr,
                             std::vector<std::pair<size_t, RecRef>> &out) {
        const Seq &full = job.contigs[(size_t)chrom].full;
        if (full.empty()) return;
        const int64_t a = end, b = std::min<int64_t>((int64_t)full.size(), end + 50);
        if (a >= b) return;
        kr.clear();
        kmer_scan(job, chrom, a, b, kr);
        for (const RecRef &x : kr)
            if (std::memcmp(x.motif, motif, 3) != 0) out.emplace_back(q, x);
    };

    // ---- pre-pass: the fold units' runs, the k-mer pieces behind 3-mer records
    // and the > 10 bp motifs.  Over the fold's survivors when the job still holds
    // them (each unit is one run of one chromosome; 32 bytes a record), else
    // over the records.
    std::optional<StageRange> sr;
    sr.emplace("bwtmi:compounds");
    std::vector<UnitPlan> plans;
    size_t NR = 0, n_pieces = 0, n_longs = 0;
    const std::shared_ptr<Survivors> held = job.survivors();   // (kept for the pass whatever another thread does)
    const Survivors *sv = held.get();
    if (sv) {
        struct Sub {
            size_t k, a, b;
            bool sorted = true;
            std::vector<std::pair<size_t, RecRef>> pieces;
            std::vector<Long> longs;
        };
        std::vector<Sub> subs;
        const size_t per = std::max<size_t>(1024, sv->size() / (size_t)(4 * std::max(1, nt)) + 1);
        for (size_t k = 0; k < sv->units(); ++k)
            for (size_t a = 0, n = sv->unit_size(k); a < n; a += per) subs.push_back({k, a, std::min(n, a + per), true, {}, {}});
        run_tasks((int64_t)subs.size(), nt, [&](int64_t t) {
            Sub &S = subs[(size_t)t];
            std::vector<RecRef> kr;
            int64_t s, e, prev = INT64_MIN;
            int32_t ml;
            if (S.a > 0) sv->span(S.k, S.a - 1, prev, e, ml);
            for (size_t i = S.a; i < S.b; ++i) {
                sv->span(S.k, i, s, e, ml);
                S.sorted = S.sorted && s >= prev;
                prev = s;
                if (!str) continue;
                if (ml > 10) S.longs.push_back({s, e, 0});
                if (ml == 3) pieces_behind(sv->unit_chrom(S.k), e, sv->view(S.k, i).motif, i, kr, S.pieces);
            }
        });
        bool sorted = true;
        for (const Sub &S : subs) sorted = sorted && S.sorted;
        if (!sorted) {
            sv = nullptr;   // (the fold leaves every unit in start order: not expected)
        } else {
            plans.resize(sv->units());
            for (size_t k = 0; k < sv->units(); ++k) {
                plans[k].unit = sv->unit_id(k);
                plans[k].n = sv->unit_size(k);
                plans[k].M.sv = sv;
                plans[k].M.su = k;
                plans[k].M.chrom = sv->unit_chrom(k);
                NR += plans[k].n;
            }
            for (Sub &S : subs) {
                UnitPlan &U = plans[S.k];
                U.found.insert(U.found.end(), S.pieces.begin(), S.pieces.end());
                U.longs.insert(U.longs.end(), S.longs.begin(), S.longs.end());
            }
        }
    }
    if (!sv) {
        const RecVec &recs = job.recs();
        NR = recs.size();
        const int PC = NR > 8192 ? 4 * std::max(1, nt) : 1;
        struct Pre {
            bool disorder = false;              // a unit after a larger one
            std::vector<size_t> ubounds;        // q: recs[q] begins a larger unit
            std::vector<int32_t> irregular;     // units with two chromosomes, or starts out of order
            std::vector<std::pair<size_t, RecRef>> pieces;
            std::vector<std::pair<size_t, Long>> longs;
        };
        std::vector<Pre> pre((size_t)PC);
        run_tasks(PC, nt, [&](int64_t t) {
            Pre &P = pre[(size_t)t];
            std::vector<RecRef> kr;
            for (size_t q = NR * (size_t)t / (size_t)PC; q < NR * (size_t)(t + 1) / (size_t)PC; ++q) {
                const Rec &r = recs[q];
                if (q > 0) {
                    const Rec &pr = recs[q - 1];
                    const int32_t u = unit_of(r), pu = unit_of(pr);
                    if (u < pu) P.disorder = true;
                    else if (u > pu) P.ubounds.push_back(q);
                    else if (r.chrom != pr.chrom || r.start < pr.start) P.irregular.push_back(u);
                }
                if (!str) continue;
                if (r.motif.size() > 10) P.longs.push_back({q, Long{r.start, r.end, 0}});
                if (r.motif.size() == 3) pieces_behind(r.chrom, r.end, r.motif.data(), q, kr, P.pieces);
            }
        });
        bool disorder = false;
        for (const Pre &P : pre) disorder = disorder || P.disorder;
        if (disorder) {   // the units' records are gathered, each unit one chunk
            std::vector<int32_t> slot((size_t)std::max(1, job.nunits), -1);
            std::vector<std::vector<const Rec *>> lists((size_t)std::max(1, job.nunits));
            for (const Rec &r : recs) lists[(size_t)unit_of(r)].push_back(&r);
            for (int32_t u = 0; u < job.nunits; ++u)
                if (!lists[(size_t)u].empty()) {
                    slot[(size_t)u] = (int32_t)plans.size();
                    plans.emplace_back();
                    plans.back().unit = u;
                    plans.back().regular = false;
                    plans.back().list.swap(lists[(size_t)u]);
                }
            for (Pre &P : pre)
                for (auto &pc : P.pieces) plans[(size_t)slot[(size_t)unit_of(recs[pc.first])]].found.push_back(pc);
        } else if (NR > 0) {
            std::vector<size_t> runs{0};
            for (const Pre &P : pre) runs.insert(runs.end(), P.ubounds.begin(), P.ubounds.end());
            runs.push_back(NR);
            std::vector<uint8_t> irr((size_t)job.nunits, 0);
            for (const Pre &P : pre)
                for (int32_t u : P.irregular) irr[(size_t)u] = 1;
            plans.resize(runs.size() - 1);
            for (size_t k = 0; k + 1 < runs.size(); ++k) {
                UnitPlan &U = plans[k];
                U.unit = unit_of(recs[runs[k]]);
                U.n = runs[k + 1] - runs[k];
                U.regular = !irr[(size_t)U.unit];
                U.M.main = recs.data() + runs[k];
                U.M.chrom = recs[runs[k]].chrom;
                if (!U.regular)
                    for (size_t q = runs[k]; q < runs[k + 1]; ++q) U.list.push_back(&recs[q]);
            }
            // pieces and long motifs arrive by record index: each goes to its run
            size_t k = 0;
            for (Pre &P : pre)
                for (auto &pc : P.pieces) {
                    while (pc.first >= runs[k + 1]) ++k;
                    plans[k].found.push_back(pc);
                }
            k = 0;
            for (Pre &P : pre)
                for (auto &lg : P.longs) {
                    while (lg.first >= runs[k + 1]) ++k;
                    if (plans[k].regular) plans[k].longs.push_back(lg.second);
                }
        }
    }
    int64_t before = 0;
    size_t n_irregular = 0;
    for (UnitPlan &U : plans) {
        const size_t n_main = U.regular ? U.n : U.list.size();
        U.base = row_base ? row_base[U.unit] : before;
        before += (int64_t)n_main;
        n_pieces += U.found.size();
        if (!U.regular) {
            ++n_irregular;
            continue;
        }
        n_longs += U.longs.size();
        for (size_t q = 0; q < U.longs.size(); ++q)
            U.longs[q].pe = q ? std::max(U.longs[q - 1].pe, U.longs[q].e) : U.longs[q].e;
        U.M.n_main = U.n;
        U.M.longs = U.longs.data();
        U.M.nl = U.longs.size();
        // the pieces by start (stably), each behind the records of equal start
        std::stable_sort(U.found.begin(), U.found.end(),
                         [](const auto &x, const auto &y) { return x.second.start < y.second.start; });
        for (size_t q = 0; q < U.found.size(); ++q) {
            U.pieces.push_back(U.found[q].second);
            U.ppos.push_back(U.M.mains_upto(U.found[q].second.start) + q);
        }
        U.M.pieces = U.pieces.data();
        U.M.ppos = U.ppos.data();
        U.M.np = U.pieces.size();
    }
    sr.reset();
    const auto t1 = clk::now();

    // ---- chunks: <= CH consecutive merged records of one unit, cut where the
    // start grows.  BWTMI_RENDER_CHUNK sets CH; by default >= 8 chunks per
    // thread while that keeps them >= 256 rows (a 40k-row shard in 8192-row
    // chunks kept 5 of 16 threads busy; in 1024-row chunks, 2 or 3 chunks a
    // thread, the last wave left threads idle)
    const int64_t n_all = (int64_t)(NR + n_pieces);
    const int64_t knob_ch = knob(KN_RENDER_CHUNK);
    const size_t CH = (size_t)(knob_ch > 0 ? knob_ch
                                           : std::max<int64_t>(256, std::min<int64_t>(8192, n_all / (8 * (int64_t)nt) + 1)));
    struct Chunk {
        size_t plan, ma, mb;
        // what a later walk from inside the chunk needs: the index each row was
        // emitted from, the rows' starts and byte offsets (both in output order,
        // which differs from the walk's only inside runs of equal start)
        std::vector<uint32_t> at;
        std::vector<size_t> off;
        std::vector<int64_t> rstart;
        size_t next = 0;
    };
    std::vector<Chunk> chunks;
    for (size_t p = 0; p < plans.size(); ++p) {
        const UnitPlan &U = plans[p];
        if (!U.regular) {
            chunks.push_back({p, 0, 0, {}, {}, {}, 0});
            continue;
        }
        const size_t N = U.M.size();
        for (size_t a = 0; a < N;) {
            size_t b = std::min(N, a + CH);
            while (b < N && U.M.start_at(b) == U.M.start_at(b - 1)) ++b;
            chunks.push_back({p, a, b, {}, {}, {}, 0});
            a = b;
        }
    }
    out.header = std::move(head);
    out.parts.clear();
    out.parts.resize(chunks.size());
    out.part_unit.resize(chunks.size());
    for (size_t q = 0; q < chunks.size(); ++q) out.part_unit[q] = plans[chunks[q].plan].unit;
    const auto t2 = clk::now();

    // ---- the pass
    sr.emplace("bwtmi:format");
    std::atomic<size_t> n_rows{0};
    size_t rewalked_chunks = 0, rewalked_rows = 0;
    // a unit that is not one sorted run: the reference's steps on one thread
    auto whole_unit = [&](const UnitPlan &U, Text &part) {
        std::vector<int32_t> order;                       // chromosomes by first record
        std::vector<std::vector<const Rec *>> by(job.contigs.size());
        for (const Rec *r : U.list) {
            if (by[(size_t)r->chrom].empty()) order.push_back(r->chrom);
            by[(size_t)r->chrom].push_back(r);
        }
        auto by_start = [](const Rec *x, const Rec *y) { return x->start < y->start; };
        std::deque<Merged> ms;
        std::deque<Walk> walks;
        std::deque<std::vector<RecRef>> pieces;
        std::deque<std::vector<size_t>> ppos;
        std::deque<std::vector<Long>> longs;
        std::vector<FRow> rows;
        for (int32_t ch : order) {
            std::vector<const Rec *> &rs = by[(size_t)ch];
            std::stable_sort(rs.begin(), rs.end(), by_start);
            pieces.emplace_back();
            ppos.emplace_back();
            longs.emplace_back();
            std::vector<std::pair<size_t, RecRef>> found;
            for (const auto &pc : U.found)
                if (pc.second.chrom == ch) found.push_back(pc);
            std::stable_sort(found.begin(), found.end(),
                             [](const auto &x, const auto &y) { return x.second.start < y.second.start; });
            for (size_t q = 0; q < found.size(); ++q) {
                pieces.back().push_back(found[q].second);
                ppos.back().push_back((size_t)(std::upper_bound(rs.begin(), rs.end(), found[q].second.start,
                                                                [](int64_t s, const Rec *r) { return s < r->start; }) -
                                               rs.begin()) + q);
            }
            if (str)
                for (const Rec *r : rs)
                    if (r->motif.size() > 10)
                        longs.back().push_back({r->start, r->end, longs.back().empty() ? r->end : std::max(longs.back().back().pe, r->end)});
            ms.emplace_back();
            Merged &M = ms.back();
            M.list = rs.data();
            M.n_main = rs.size();
            M.pieces = pieces.back().data();
            M.ppos = ppos.back().data();
            M.np = pieces.back().size();
            M.longs = longs.back().data();
            M.nl = longs.back().size();
            M.chrom = ch;
            walks.emplace_back(job, M, 0, M.size());
            Walk &w = walks.back();
            for (size_t i = 0; i < M.size();) {
                if (str) i = w.step(i);
                else w.plain(i++);
            }
        }
        for (const Walk &w : walks) w.resolve(rows);
        // sorted(key=(start, end)) within the unit (bwt.py:4150)
        std::stable_sort(rows.begin(), rows.end(), [](const FRow &x, const FRow &y) {
            return x.r->start != y.r->start ? x.r->start < y.r->start : x.r->end < y.r->end;
        });
        Out o;
        format_rows(o, job, fmt, rows, U.base, nullptr);
        part = o.finish();
        n_rows.fetch_add(rows.size(), std::memory_order_relaxed);
    };
    auto chunk_task = [&](size_t ck) {
        Chunk &C = chunks[ck];
        const UnitPlan &U = plans[C.plan];
        if (!U.regular) {
            whole_unit(U, out.parts[ck]);
            return;
        }
        Walk w(job, U.M, C.ma, C.mb - C.ma);
        size_t i = C.ma;
        while (i < C.mb) {
            if (str) i = w.step(i);
            else w.plain(i++);
        }
        C.next = i;
        std::vector<FRow> rows;
        rows.reserve(w.rows.size());
        w.resolve(rows);
        order_equal_starts(rows);
        Out o;
        format_rows(o, job, fmt, rows, U.base + (int64_t)C.ma, str ? &C.off : nullptr);
        out.parts[ck] = o.finish();
        if (str) {
            C.at.swap(w.at);
            C.rstart.reserve(rows.size());
            for (const FRow &r : rows) C.rstart.push_back(r.r->start);
        }
        n_rows.fetch_add(rows.size(), std::memory_order_relaxed);
    };
    // the true walk enters chunk ck at ti (inside it, not at its first index)
    auto rewalk = [&](size_t ck, size_t ti) -> size_t {
        Chunk &C = chunks[ck];
        const UnitPlan &U = plans[C.plan];
        Walk w(job, U.M, ti);
        size_t i = ti, keep = C.at.size();   // keep: the first row whose bytes stay
        std::vector<FRow> rows;
        while (i < C.mb) {
            const uint32_t rel = (uint32_t)(i - C.ma);
            const size_t q = (size_t)(std::lower_bound(C.at.begin(), C.at.end(), rel) - C.at.begin());
            // q >= 1: the first walk stepped from the chunk's first index, before ti
            if (q < C.at.size() && C.at[q] == rel && C.rstart[q] > C.rstart[q - 1] &&
                (w.rows.empty() || C.rstart[q] > w.ref(w.rows.back().r)->start)) {
                keep = q;
                break;
            }
            i = w.step(i);
        }
        w.resolve(rows);
        order_equal_starts(rows);
        Out o;
        format_rows(o, job, fmt, rows, 0, nullptr);
        const Text &old = out.parts[ck];
        if (keep < C.at.size()) o.put(old.data() + C.off[keep], (int64_t)(old.size() - C.off[keep]));
        n_rows.fetch_add(rows.size(), std::memory_order_relaxed);
        n_rows.fetch_sub(keep, std::memory_order_relaxed);
        out.parts[ck] = o.finish();
        ++rewalked_chunks;
        rewalked_rows += rows.size();
        return keep < C.at.size() ? C.next : i;
    };
    // chunks are committed in order, by whichever thread finds the next one
    // done: a part is final (on_part) once the walk before it is known
    std::mutex mu;
    std::vector<uint8_t> done(chunks.size(), 0);
    size_t frontier = 0, ti = 0;
    bool committing = false;
    auto commit = [&](size_t ck) {
        Chunk &C = chunks[ck];
        if (str && plans[C.plan].regular) {
            if (C.ma == 0) ti = 0;
            if (ti >= C.mb) {   // the walk stepped over the whole chunk
                n_rows.fetch_sub(C.at.size(), std::memory_order_relaxed);
                rewalked_chunks += 1;
                out.parts[ck] = Text();
            } else if (ti != C.ma) {
                ti = rewalk(ck, ti);
            } else {
                ti = C.next;
            }
            std::vector<uint32_t>().swap(C.at);
            std::vector<size_t>().swap(C.off);
            std::vector<int64_t>().swap(C.rstart);
        }
        if (on_part) (*on_part)(ck);
    };
    // BWTMI_STATS=3: per-chunk timeline (thread, walk + formatting, commit) of the pass
    struct Tl { double a, b, c0, c1; size_t th, cth; };
    std::vector<Tl> tl(stats_on(3) ? chunks.size() : 0);
    auto now_ms = [t2] { return std::chrono::duration<double, std::milli>(clk::now() - t2).count(); };
    auto this_th = [] { return std::hash<std::thread::id>()(std::this_thread::get_id()); };
    run_tasks((int64_t)chunks.size(), nt, [&](int64_t ck) {
        if (!tl.empty()) { tl[(size_t)ck].a = now_ms(); tl[(size_t)ck].th = this_th(); }
        chunk_task((size_t)ck);
        if (!tl.empty()) tl[(size_t)ck].b = now_ms();
        std::unique_lock<std::mutex> lk(mu);
        done[(size_t)ck] = 1;
        if (committing) return;
        committing = true;
        while (frontier < chunks.size() && done[frontier]) {
            const size_t f = frontier;
            lk.unlock();
            if (!tl.empty()) { tl[f].c0 = now_ms(); tl[f].cth = this_th(); }
            commit(f);
            if (!tl.empty()) tl[f].c1 = now_ms();
            lk.lock();
            ++frontier;
        }
        committing = false;
    });
    sr.reset();
    const auto t3 = clk::now();
    if (!tl.empty()) {
        std::map<size_t, std::pair<double, double>> busy;   // thread -> (walk + formatting, commit with on_part)
        double first = 1e30, last = 0, lastfmt = 0;
        for (const Tl &x : tl) {
            busy[x.th].first += x.b - x.a;
            busy[x.cth].second += x.c1 - x.c0;
            first = std::min(first, x.a);
            last = std::max(last, x.c1);
            lastfmt = std::max(lastfmt, x.b);
        }
        std::string per;
        for (auto &kv : busy) per += " " + std::to_string((int)(kv.second.first * 100) / 100.0).substr(0, 4) + "/" +
                                     std::to_string((int)(kv.second.second * 100) / 100.0).substr(0, 4);
        std::fprintf(stderr, "  format timeline: %zu chunks, first start %.2f, last format end %.2f, last end %.2f ms; "
                     "threads (format/commit ms):%s\n", tl.size(), first, lastfmt, last, per.c_str());
    }
    job.stage_ms[6] = std::chrono::duration<double, std::milli>(t3 - t0).count();
    if (stats_on()) {
        auto d = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        if (str)
            std::fprintf(stderr, "  compounds: pre-pass %.1f ms (%zu pieces, %zu long motifs; %zu units, %zu not one sorted run); "
                         "walked again from inside: %zu chunks, %zu rows\n", d(t0, t1), n_pieces, n_longs, plans.size(),
                         n_irregular, rewalked_chunks, rewalked_rows);
        std::fprintf(stderr, "  render: pre-pass %.1f chunking %.1f pass %.1f ms (%zu chunks, %zu rows)\n", d(t0, t1),
                     d(t1, t2), d(t2, t3), chunks.size(), n_rows.load());
    }
}

std::vector<Text> render_parts(Job &job, int fmt) {
    Rendered r;
    render_rows(job, fmt, nullptr, r);
    std::vector<Text> parts;
    parts.reserve(r.parts.size() + 1);
    parts.emplace_back(r.header.data(), r.header.size());
    for (auto &p : r.parts) parts.push_back(std::move(p));
    return parts;
}

std::string render(Job &job, int fmt) {
    std::vector<Text> parts = render_parts(job, fmt);
    size_t tot = 0;
    for (auto &p : parts) tot += p.size();
    std::string s;
    s.reserve(tot);
    for (auto &p : parts) s.append(p.data(), p.size());
    return s;
}

}  // namespace bwtmi
