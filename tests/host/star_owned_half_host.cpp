// Host build of salve_amd/csrc/star_delaunay.h + star_local.h (the SAME source the HIP kernel compiles) for the owned-half stop
// rule: the lean walk of every site is stopped after k = 0, 1, 2, ... steps and handed to the general walk, as the kernel does
// when a lean walk gives up, and what the two emitted together is compared with the triangles the site owns.  Test-only.
#include <algorithm>
#include <array>
#include <cstring>
#include <vector>
#include "../../salve_amd/csrc/star_delaunay.h"
#include "../../salve_amd/csrc/star_table.h"
#include "../../salve_amd/csrc/star_local.h"

static const int8_t* host_table() {
    static SdTable t;
    static bool ok = sdt_build(&t);
    return ok ? &t.off[0][0][0] : nullptr;
}

typedef std::array<int, 6> Tri;
struct Collect {
    std::vector<Tri>* out;
    int bad;   // triangles not handed over as (s, b, c) counter-clockwise
    int sx, sy;
    void operator()(int ax, int ay, int bx, int by, int cx, int cy) {
        if (ax != sx || ay != sy || sd_orient(ax, ay, bx, by, cx, cy) <= 0) bad++;
        // canonical form: s first, then the other two in raster order
        Tri t = {ax, ay, bx, by, cx, cy};
        if (sd_before(cx, cy, bx, by)) t = {ax, ay, cx, cy, bx, by};
        out->push_back(t);
    }
};

// ref_tri: the oracle's triangles, 6 ints each (any vertex order).  For every site and every k: lean walk for k steps, then the
// general walk from that state; lean + general must emit the site's owned triangles, each exactly once.
// stats: [0] hand-overs checked, [1] of them resumed (not fresh): [2] with dir = +1, [3] -1, [4] +2 (not a half walk), [5] -2, [6] as half
//        walks; [7] lean walks that finished by themselves.   fail: [0] x, [1] y, [2] k of the first failure.
// Returns the number of (site, k) pairs that failed, or a negative error.
extern "C" int owned_half_handover(const int* xs, const int* ys, int n, int H, int W, const int* ref_tri, int nref, int use_table, int use_cache,
                                   long long* stats, int* fail) {
    if (use_table && !host_table()) return -3;
    static unsigned long long cache[SD_CACHE_SIZE];
    memset(cache, 0, sizeof(cache));
    const int wpr = (W + 31) / 32;
    std::vector<uint32_t> occ((size_t)H * wpr, 0);
    std::vector<int16_t> rmin(H, (int16_t)W), rmax(H, (int16_t)-1);
    int bx0 = W, bx1 = -1, by0 = H, by1 = -1;
    for (int i = 0; i < n; i++) {
        occ[(size_t)ys[i] * wpr + (xs[i] >> 5)] |= 1u << (xs[i] & 31);
        if (xs[i] < rmin[ys[i]]) rmin[ys[i]] = (int16_t)xs[i];
        if (xs[i] > rmax[ys[i]]) rmax[ys[i]] = (int16_t)xs[i];
        bx0 = std::min(bx0, xs[i]); bx1 = std::max(bx1, xs[i]); by0 = std::min(by0, ys[i]); by1 = std::max(by1, ys[i]);
    }
    SdGrid g = {H, W, wpr, occ.data(), rmin.data(), rmax.data(), 0, 1, use_table ? host_table() : nullptr, bx0, bx1, by0, by1, use_cache ? cache : nullptr};
    // the oracle's triangles by owner (raster-first vertex), canonical form
    std::vector<Tri> ref;
    for (int t = 0; t < nref; t++) {
        std::array<std::array<int, 2>, 3> v;
        for (int q = 0; q < 3; q++) v[q] = {ref_tri[6 * t + 2 * q], ref_tri[6 * t + 2 * q + 1]};
        std::sort(v.begin(), v.end(), [](const std::array<int, 2>& a, const std::array<int, 2>& b) { return sd_before(a[0], a[1], b[0], b[1]); });
        ref.push_back(Tri{v[0][0], v[0][1], v[1][0], v[1][1], v[2][0], v[2][1]});
    }
    std::sort(ref.begin(), ref.end());
    int failed = 0;
    for (int i = 0; i < n; i++) {
        const int sx = xs[i], sy = ys[i];
        const auto lo = std::lower_bound(ref.begin(), ref.end(), Tri{sx, sy, INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN});
        const auto hi = std::upper_bound(ref.begin(), ref.end(), Tri{sx, sy, INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX});
        const std::vector<Tri> want(lo, hi);
        for (int k = 0;; k++) {
            std::vector<Tri> mine;
            Collect c = {&mine, 0, sx, sy};
            SdLean ls;
            int r = sdl_lean_begin(ls, g, sx, sy);
            int it = 0;
            while (r == SDL_LEAN_CONTINUE && it < k) { r = sdl_lean_step(ls, g, c); it++; }
            int steps = 0;
            if (r == SDL_LEAN_DONE) {
                stats[7]++;
            } else {
                const bool fresh = ls.n0x == SDL_NONE || g.tab == nullptr;   // gave up in sdl_lean_begin: nothing to take over
                stats[0]++;
                if (!fresh) {
                    stats[1]++;
                    stats[ls.half ? 6 : ls.dir == 1 ? 2 : ls.dir == -1 ? 3 : ls.dir == 2 ? 4 : 5]++;
                }
                steps = fresh ? sd_star(g, sx, sy, c) : sd_star_resume(g, sx, sy, ls.ax, ls.ay, ls.dir, ls.half, ls.n0x, ls.n0y, c);
            }
            std::sort(mine.begin(), mine.end());
            if (steps < 0 || c.bad || mine != want) {
                if (!failed) { fail[0] = sx; fail[1] = sy; fail[2] = k; }
                failed++;
            }
            if (r != SDL_LEAN_CONTINUE) break;   // the lean walk finished, or gave up, by itself: there is no later state
        }
    }
    return failed;
}
