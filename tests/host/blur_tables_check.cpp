// Host checker for blur_tables() (csrc/blur.hip): reads kernels from a file, rebuilds each kernel's tables and reports, one
// JSON line per record, every property of the tables the launchers and the tap loops rely on that does not hold, plus the
// route facts the launchers derive from the tables.  Built by tests/test_blur_tables_cpu.py (host only, under the address
// and undefined-behaviour sanitizers) and run as a child process; nothing here touches a device.
//
// Input: records of  int32 ks, int32 mode, ks * ks float32 (row-major), back to back.
// The translation unit IS blur.hip, so its file-static helpers (taps_swc, make_geom, sep_adj_sym_ok) and the tile
// constants are the ones the library is built from.
#include "blur.hip"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace dpsx;

namespace {

struct Report {
    std::vector<std::string> viol;
    void fail(const char *what, int a = 0, int b = 0)
    {
        char buf[160];
        std::snprintf(buf, sizeof buf, "%s(%d,%d)", what, a, b);
        if (viol.size() < 8) viol.push_back(buf);
    }
};

bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// scatter a run table back onto the ks x ks grid: sign = +1 forward (tap at dy0 + q, dx), -1 adjoint (negated offsets)
void scatter(const std::vector<TapRun> &runs, const int (&nrun)[4], int ks, int sign, const std::vector<float> &k,
             Report &rep, const char *tag)
{
    const int R = ks / 2;
    std::vector<float> dense((size_t)ks * ks, 0.0f);
    std::vector<char> set((size_t)ks * ks, 0);
    size_t at = 0;
    for (int c = 0; c < 4; ++c) {
        const int L = (c & 1) ? 2 : 4;
        for (int n = 0; n < nrun[c] && at < runs.size(); ++n, ++at) {
            const TapRun &r = runs[at];
            for (int q = 0; q < L; ++q) {
                if (r.w[q] == 0.0f) continue;
                const int i = sign * (r.dy0 + q) + R, j = sign * r.dx + R;
                if (i < 0 || i >= ks || j < 0 || j >= ks) { rep.fail((std::string(tag) + ":off_grid").c_str(), i, j); continue; }
                if (set[(size_t)i * ks + j]) rep.fail((std::string(tag) + ":tap_twice").c_str(), i, j);
                set[(size_t)i * ks + j] = 1;
                dense[(size_t)i * ks + j] = r.w[q];
            }
        }
    }
    for (int i = 0; i < ks; ++i)
        for (int j = 0; j < ks; ++j) {
            const float want = k[(size_t)i * ks + j];
            const bool ok = want == 0.0f ? !set[(size_t)i * ks + j] : same_bits(dense[(size_t)i * ks + j], want);
            if (!ok) rep.fail((std::string(tag) + ":dense_differs").c_str(), i, j);
        }
}

int ceil4(int v) { return (v + 3) / 4 * 4; }

void check_record(long idx, int ks, int mode, const std::vector<float> &k)
{
    const BlurTables t = blur_tables(k.data(), ks, mode);
    Report rep;
    const int R = ks / 2;
    // ---- run tables
    int total = 0;
    for (int c = 0; c < 4; ++c) {
        total += t.nrun[c];
        if (t.nrun[c] % 2) rep.fail("odd_class", c, t.nrun[c]);
        if (t.nrun[c] < 0) rep.fail("negative_class", c, t.nrun[c]);
    }
    if ((size_t)total != t.fwd.size() || (size_t)total != t.adj.size()) rep.fail("run_count", total, (int)t.fwd.size());
    if ((size_t)total == t.fwd.size() && (size_t)total == t.adj.size()) {
        size_t at = 0;
        for (int c = 0; c < 4; ++c) {
            const int L = (c & 1) ? 2 : 4;
            int pos = 0, neg = 0;
            for (int n = 0; n < t.nrun[c]; ++n, ++at) {
                const TapRun &f = t.fwd[at], &a = t.adj[at];
                if ((f.dx & 1) != (c >> 1)) rep.fail("fwd_parity", c, f.dx);
                if ((a.dx & 1) != (c >> 1)) rep.fail("adj_parity", c, a.dx);
                for (int q = L; q < 4; ++q)
                    if (f.w[q] != 0.0f || a.w[q] != 0.0f) rep.fail("slot_beyond_L", c, q);
                // ---- halos: the staged window of every run
                if (f.dy0 < -t.halo_t || f.dy0 + L - 1 > t.halo_b) rep.fail("fwd_rows_outside_halo", f.dy0, L);
                if (f.dx < -t.halo_l || f.dx > t.halo_r) rep.fail("fwd_col_outside_halo", f.dx, 0);
                if (a.dy0 < -t.halo_b || a.dy0 + L - 1 > t.halo_t) rep.fail("adj_rows_outside_halo", a.dy0, L);
                if (a.dx < -t.halo_r || a.dx > t.halo_l) rep.fail("adj_col_outside_halo", a.dx, 0);
                // ---- adjoint ordering
                if (n > 0 && a.dx > t.adj[at - 1].dx) rep.fail("adj_not_sorted", c, n);
                pos += a.dx >= 1;
                neg += a.dx <= -1;
            }
            if (pos != t.nrun_adj_pos[c]) rep.fail("adj_pos_count", c, t.nrun_adj_pos[c]);
            if (neg != t.nrun_adj_neg[c]) rep.fail("adj_neg_count", c, t.nrun_adj_neg[c]);
        }
        scatter(t.fwd, t.nrun, ks, +1, k, rep, "fwd");
        scatter(t.adj, t.nrun, ks, -1, k, rep, "adj");
    }
    if (t.halo_t + t.halo_b < 3) rep.fail("halo_rows_below_3", t.halo_t, t.halo_b);
    if (t.halo_t < 0 || t.halo_b < 0 || t.halo_l < 0 || t.halo_r < 0) rep.fail("negative_halo", t.halo_t, t.halo_l);
    if (t.halo_l % 4 || t.halo_r % 4) rep.fail("halo_cols_not_x4", t.halo_l, t.halo_r);
    // ---- scalars
    int reach = 0;
    bool any = false;
    double mass = 0.0;
    for (int i = 0; i < ks; ++i)
        for (int j = 0; j < ks; ++j)
            if (k[(size_t)i * ks + j] != 0.0f) {
                any = true;
                reach = std::max(reach, std::max(std::abs(i - R), std::abs(j - R)));
                mass += std::fabs((double)k[(size_t)i * ks + j]);
            }
    if (t.radius != R) rep.fail("radius", t.radius, R);
    if (t.reach != reach) rep.fail("reach", t.reach, reach);
    if (t.radius4 != std::max(4, ceil4(reach))) rep.fail("radius4", t.radius4, reach);
    // ---- separable branch
    if (t.separable && (mode == DPSX_BLUR_FORCE_TAPS || !any)) rep.fail("separable_not_allowed", mode, any);
    if (t.separable) {
        const int r4 = t.radius4;
        for (int d = 0; d <= 2 * kMaxRadius; ++d)
            if (std::abs(d - r4) > reach && (t.sep.v[d] != 0.0f || t.sep.h[d] != 0.0f)) rep.fail("sep_beyond_reach", d, r4);
        double dist = 0.0;
        for (int i = 0; i < ks; ++i)
            for (int j = 0; j < ks; ++j) {
                const int di = i - R, dj = j - R;
                const double v = std::abs(di) <= reach ? (double)t.sep.v[r4 + di] : 0.0;
                const double h = std::abs(dj) <= reach ? (double)t.sep.h[r4 + dj] : 0.0;
                dist += std::fabs(v * h - (double)k[(size_t)i * ks + j]);
            }
        if (!(dist <= 1e-6 * mass)) rep.fail("sep_outside_l1_bound", (int)(dist / mass * 1e9), 0);
    }
    // ---- route facts, as the launchers derive them
    const TapGeom gf = make_geom(t.halo_t, t.halo_b, t.halo_l, t.halo_r);                 // forward tap list
    const AdjReach ar{t.halo_b, t.halo_t, t.halo_r, t.halo_l};                            // one-launch adjoint
    const TapGeom ga = make_geom(std::max(ar.t, 11), std::max(ar.b, 11), std::max(ar.l, 4), std::max(ar.r, 4));
    const int halo_units = (gf.t + gf.b) * ((TW + gf.l + gf.r) / 4) + TH * ((gf.l + gf.r) / 4);
    const int hmax = std::max(ar.l, ar.r);
    const bool strip16 = hmax <= 14;
    const bool multipass = hmax > (strip16 ? 14 : 30);
    int sym = -1;
    if (t.separable) {
        BlurArgs a{};
        a.h = 2 * TH; a.w = 2 * TW; a.tiles_x = 2; a.tiles_y = 2;
        sym = sep_adj_sym_ok(t, a) ? 1 : 0;
    }
    std::printf("{\"i\": %ld, \"ks\": %d, \"mode\": %d, \"separable\": %s, \"reach\": %d, \"radius4\": %d, "
                "\"halo\": [%d, %d, %d, %d], \"nrun\": [%d, %d, %d, %d], \"swc_fwd\": %d, \"swc_adj\": %d, "
                "\"nhb2\": %s, \"strip16\": %s, \"multipass\": %s, \"sym\": %s, \"empty\": [%s, %s, %s, %s], \"viol\": [",
                idx, ks, mode, t.separable ? "true" : "false", t.reach, t.radius4, t.halo_t, t.halo_b, t.halo_l, t.halo_r,
                t.nrun[0], t.nrun[1], t.nrun[2], t.nrun[3], taps_swc(gf, true), taps_swc(ga, true),
                halo_units <= 2 * NT ? "true" : "false", strip16 ? "true" : "false", multipass ? "true" : "false",
                sym < 0 ? "null" : (sym ? "true" : "false"), t.nrun[0] ? "false" : "true", t.nrun[1] ? "false" : "true",
                t.nrun[2] ? "false" : "true", t.nrun[3] ? "false" : "true");
    for (size_t v = 0; v < rep.viol.size(); ++v) std::printf("%s\"%s\"", v ? ", " : "", rep.viol[v].c_str());
    std::printf("]}\n");
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s RECORDS\n", argv[0]);
        return 2;
    }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    long idx = 0;
    for (;; ++idx) {
        int32_t head[2];
        const size_t got = std::fread(head, sizeof(int32_t), 2, f);
        if (got == 0) break;
        const int ks = head[0], mode = head[1];
        if (got != 2 || ks < 1 || ks > 2 * kMaxRadius + 1 || ks % 2 == 0) {
            std::fprintf(stderr, "record %ld: bad header\n", idx);
            return 2;
        }
        std::vector<float> k((size_t)ks * ks);
        if (std::fread(k.data(), sizeof(float), k.size(), f) != k.size()) {
            std::fprintf(stderr, "record %ld: truncated\n", idx);
            return 2;
        }
        check_record(idx, ks, mode, k);
    }
    std::fclose(f);
    return 0;
}
