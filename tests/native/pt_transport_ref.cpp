/*
 * pt_transport_ref.cpp — an independent float64 estimator of path B's light transport.
 *
 * TEST INFRASTRUCTURE ONLY: a stand-alone program, built with g++ by tests/transport_ref.py.  Files in, file out.
 * It includes nothing from oracle/ or raytracing_engine_amd/csrc/ and calls nothing of theirs; it is written from the physics
 * and from the prose of DESIGN §6.1, §6.4 and §6.11: double precision throughout, Moeller-Trumbore over ALL triangles with
 * the closest t > 0 (no tree), libm sin/cos, its own generator (splitmix64 -> 53-bit doubles) and textbook formulas.
 *
 * THE ESTIMATOR is brute force: NO next-event estimation.  A path is followed until it leaves the scene or meets an emitter.
 *   Lambert   continue in a cosine-distributed direction around the normal that faces the ray, T *= albedo
 *   mirror    reflect, T *= albedo
 *   glass     unpolarised Fresnel F from Snell's law; the ray enters iff it arrives on the side e1 x e2 points to; reflect
 *             with probability F (always at total internal reflection), otherwise refract; T *= albedo in both cases
 *   origins   offset by ray_eps along the facing normal: inward for a refracted ray, outward otherwise
 *   emitters  two-sided, they end the path
 *
 * THE TRUNCATION that makes the expectation equal the specification's for `bounces` = B.  The specification gathers light in
 * two ways: a camera ray or a ray that leaves a delta vertex (mirror, glass) counts the emitter it hits, and a Lambert vertex
 * counts one emitter through a shadow ray (next-event estimation), at every depth d <= B, while a path hitting an emitter after
 * a Lambert vertex counts nothing.  Either way an emitter that is reached as vertex d of a path counts exactly once, as long
 * as the vertex before it may still gather: so here, with vertices at depth 0 .. B + 1,
 *   a miss adds T * sky only at depth <= B                      (the specification traces no ray from depth B onwards)
 *   an emitter hit at depth d adds T * Le if d <= B, or if d == B + 1 and the vertex at depth B was Lambert
 *                                                               (that is the next-event estimate of the vertex at depth B)
 *   a delta vertex at depth B ends the path with nothing added  (the specification's rule, §6.11)
 *
 * NOT MODELLED, on purpose: the shadow segment's 0.999 cut, the 2^-24 grid of the specification's random numbers and its
 * rule for a light closer than 2^-37.  The validation scenes keep these far below the tolerance.
 *
 * SAMPLING.  The work is cut into units (batch b, pixel p) of `spp` paths; unit (b, p) draws from a generator keyed by
 * (seed, b, p) alone and writes to its own slot, and the slots are reduced in index order by one thread: a run is reproducible
 * for a seed and does not depend on the number of threads.  Every batch holds `spp` paths of every pixel, so a batch mean of
 * a cell is an independent estimate of the cell, and the standard error is the deviation of the batch means / sqrt(batches).
 * The per-path deviation is the pooled deviation of a path's value within its pixel (what sqrt(paths) * standard error
 * estimates for an estimator that gives every pixel equally many paths, as this one and the specification's do).
 *
 * usage: pt_transport_ref SCENE PARAMS OUT [threads = 16]
 *   SCENE   float64, 17 per triangle: v0 v1 v2 (9), albedo (3), emission (3), kind (0 Lambert, 1 mirror, 2 glass), index
 *   PARAMS  float64 x 24: width height cells_x cells_y bounces seed batches spp ratio_x ratio_y rot(x y z w) pos(3) sky(3)
 *           ray_eps only_depth (-1: all; d >= 0: only what is gathered at vertex depth d counts) pad pad
 *   OUT     float64: paths, cells_y, cells_x, depths = B + 2, then mean / standard error / per-path deviation per cell and
 *           channel (3 arrays of cells_y * cells_x * 3), the same three for the frame (3 x 3), then the frame mean split by
 *           the depth of the vertex that gathered it (depths x 3)
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
#include <atomic>

#include "ref_io.h"

struct V { double x, y, z; };
static inline V operator+(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static inline V operator-(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static inline V operator*(V a, double s) { return {a.x * s, a.y * s, a.z * s}; }
static inline double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static inline V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static inline V unit(V a) { return a * (1.0 / std::sqrt(dot(a, a))); }

struct Tri { V v0, e1, e2, n; double albedo[3], emission[3]; int kind; double ior; bool light; };

struct Rng { /* splitmix64 */
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    double uniform() { return (double)(next() >> 11) * 0x1p-53; } /* [0, 1) */
};
static Rng keyed(uint64_t seed, uint64_t batch, uint64_t pixel) {
    Rng a{seed};
    Rng b{a.next() ^ (batch * 0xd1342543de82ef95ull)};
    Rng c{b.next() ^ (pixel * 0xaf251af3b0f025b5ull)};
    return Rng{c.next()};
}

struct Params {
    int width, height, cells_x, cells_y, bounces, batches, spp, only_depth;
    uint64_t seed;
    double ratio[2], rot[4], pos[3], sky[3], ray_eps;
};

/* Moeller-Trumbore, both sides; the closest t > 0 over all triangles */
static int closest(const std::vector<Tri>& tris, V o, V d, double* t_out) {
    int best = -1;
    double bt = INFINITY;
    for (size_t i = 0; i < tris.size(); i++) {
        const Tri& T = tris[i];
        const V p = cross(d, T.e2);
        const double det = dot(T.e1, p);
        if (det == 0.0) continue;
        const double inv = 1.0 / det;
        const V s = o - T.v0;
        const double u = dot(s, p) * inv;
        if (u < 0.0 || u > 1.0) continue;
        const V q = cross(s, T.e1);
        const double v = dot(d, q) * inv;
        if (v < 0.0 || u + v > 1.0) continue;
        const double t = dot(T.e2, q) * inv;
        if (t > 0.0 && t < bt) { bt = t; best = (int)i; }
    }
    *t_out = bt;
    return best;
}

static V rotate(const double q[4], V v) { /* unit quaternion (x, y, z, w): v + 2 w (u x v) + 2 u x (u x v) */
    const V u{q[0], q[1], q[2]};
    const V c = cross(u, v);
    return v + c * (2.0 * q[3]) + cross(u, c) * 2.0;
}

static V cosine_direction(V n, Rng& g) { /* density cos / pi around the unit vector n */
    const double u1 = g.uniform(), u2 = g.uniform();
    const double r = std::sqrt(u1), phi = 2.0 * M_PI * u2;
    const V a = std::fabs(n.x) > 0.6 ? V{0.0, 1.0, 0.0} : V{1.0, 0.0, 0.0};
    const V t = unit(cross(a, n)), b = cross(n, t);
    return t * (r * std::cos(phi)) + b * (r * std::sin(phi)) + n * std::sqrt(1.0 - u1);
}

/* one path through pixel (px, py); what the vertex at depth d gathers goes to by_depth[d] */
static void path(const std::vector<Tri>& tris, const Params& P, int px, int py, Rng& g, double L[3], double* by_depth) {
    const double nx = ((px + g.uniform()) * 2.0 / P.width - 1.0) * P.ratio[0];
    const double ny = ((py + g.uniform()) * 2.0 / P.height - 1.0) * P.ratio[1];
    V d = unit(rotate(P.rot, V{nx, 1.0, ny}));
    V o{P.pos[0], P.pos[1], P.pos[2]};
    double T[3] = {1.0, 1.0, 1.0};
    L[0] = L[1] = L[2] = 0.0;
    const int B = P.bounces;
    bool after_lambert = false;
    for (int depth = 0; depth <= B + 1; depth++) {
        double t;
        const int i = closest(tris, o, d, &t);
        const double* gathered = nullptr;
        if (i < 0) {
            if (depth <= B) gathered = P.sky;
        } else if (tris[i].light) {
            if (depth <= B || after_lambert) gathered = tris[i].emission;
        }
        if (gathered) {
            if (P.only_depth < 0 || P.only_depth == depth)
                for (int k = 0; k < 3; k++) L[k] += T[k] * gathered[k];
            for (int k = 0; k < 3; k++) by_depth[3 * depth + k] += T[k] * gathered[k];
        }
        if (i < 0 || tris[i].light || depth == B + 1) return;
        const Tri& S = tris[i];
        const bool enters = dot(S.n, d) < 0.0; /* the ray arrives on the side e1 x e2 points to */
        const V n = enters ? S.n : S.n * -1.0; /* the normal that faces the ray */
        const V p = o + d * t;
        bool inward = false;
        if (S.kind == 0) {
            d = cosine_direction(n, g);
            after_lambert = true;
        } else {
            if (depth == B) return; /* a delta vertex at the last depth gathers nothing */
            const double ci = -dot(n, d);
            bool reflect = true;
            if (S.kind == 2) {
                const double n1 = enters ? 1.0 : S.ior, n2 = enters ? S.ior : 1.0;
                const double eta = n1 / n2, s2 = eta * eta * (1.0 - ci * ci);
                if (s2 < 1.0) {
                    const double ctr = std::sqrt(1.0 - s2);
                    const double rs = (n1 * ci - n2 * ctr) / (n1 * ci + n2 * ctr), rp = (n1 * ctr - n2 * ci) / (n1 * ctr + n2 * ci);
                    const double F = 0.5 * (rs * rs + rp * rp);
                    if (!(g.uniform() < F)) {
                        reflect = false;
                        d = unit(d * eta + n * (eta * ci - ctr));
                        inward = true;
                    }
                }
            }
            if (reflect) d = unit(d + n * (2.0 * ci));
            after_lambert = false;
        }
        o = p + n * (inward ? -P.ray_eps : P.ray_eps);
        for (int k = 0; k < 3; k++) T[k] *= S.albedo[k];
    }
}

struct Moments { double mean[3], se[3], sd[3]; };

/* the pixels [x0, x1) x [y0, y1): sums[(b * pixels + p) * 6 + (k | 3 + k)] = sum and sum of squares of unit (b, p), channel k */
static Moments reduce(const std::vector<double>& sums, const Params& P, int x0, int x1, int y0, int y1) {
    Moments m;
    const int pixels = P.width * P.height, count = (x1 - x0) * (y1 - y0);
    for (int k = 0; k < 3; k++) {
        double total = 0.0, within = 0.0;
        for (int b = 0; b < P.batches; b++) {
            double s = 0.0;
            for (int y = y0; y < y1; y++)
                for (int x = x0; x < x1; x++) s += sums[((size_t)b * pixels + (size_t)y * P.width + x) * 6 + k];
            const double bm = s / ((double)count * P.spp);
            total += bm;
        }
        const double mean = total / P.batches;
        double var = 0.0;
        if (P.batches > 1) { /* second pass: no cancellation */
            for (int b = 0; b < P.batches; b++) {
                double s = 0.0;
                for (int y = y0; y < y1; y++)
                    for (int x = x0; x < x1; x++) s += sums[((size_t)b * pixels + (size_t)y * P.width + x) * 6 + k];
                const double dm = s / ((double)count * P.spp) - mean;
                var += dm * dm;
            }
            var /= (P.batches - 1);
        }
        for (int y = y0; y < y1; y++)
            for (int x = x0; x < x1; x++) {
                double s = 0.0, s2 = 0.0;
                for (int b = 0; b < P.batches; b++) {
                    const double* u = &sums[((size_t)b * pixels + (size_t)y * P.width + x) * 6];
                    s += u[k];
                    s2 += u[3 + k];
                }
                const double n = (double)P.batches * P.spp, pm = s / n;
                const double v = s2 / n - pm * pm;
                within += (v > 0.0 ? v : 0.0) * n / (n - 1.0);
            }
        m.mean[k] = mean;
        m.se[k] = std::sqrt(var / P.batches);
        m.sd[k] = std::sqrt(within / count);
    }
    return m;
}

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: pt_transport_ref SCENE PARAMS OUT [threads]\n"); return 2; }
    std::vector<double> sc, pr;
    if (!ref::read_all(argv[1], sc) || !ref::read_all(argv[2], pr)) { std::fprintf(stderr, "bad input files\n"); return 2; }
    int threads = argc > 4 ? std::atoi(argv[4]) : 16;
    if (threads < 1) threads = 1;
    if (sc.empty() || sc.size() % 17 != 0 || pr.size() != 24) { std::fprintf(stderr, "bad input files\n"); return 2; }
    Params P;
    P.width = (int)pr[0]; P.height = (int)pr[1]; P.cells_x = (int)pr[2]; P.cells_y = (int)pr[3]; P.bounces = (int)pr[4];
    P.seed = (uint64_t)pr[5]; P.batches = (int)pr[6]; P.spp = (int)pr[7];
    P.ratio[0] = pr[8]; P.ratio[1] = pr[9];
    for (int k = 0; k < 4; k++) P.rot[k] = pr[10 + k];
    for (int k = 0; k < 3; k++) { P.pos[k] = pr[14 + k]; P.sky[k] = pr[17 + k]; }
    P.ray_eps = pr[20]; P.only_depth = (int)pr[21];
    if (P.width < 1 || P.height < 1 || P.cells_x < 1 || P.cells_y < 1 || P.width % P.cells_x || P.height % P.cells_y || P.bounces < 0 ||
        P.batches < 1 || P.spp < 1 || (double)P.width * P.height * P.batches > 1e8) { std::fprintf(stderr, "bad parameters\n"); return 2; }
    const double qn = std::sqrt(P.rot[0] * P.rot[0] + P.rot[1] * P.rot[1] + P.rot[2] * P.rot[2] + P.rot[3] * P.rot[3]);
    if (!(qn > 0.0)) { std::fprintf(stderr, "bad rotation\n"); return 2; }
    for (int k = 0; k < 4; k++) P.rot[k] /= qn;

    std::vector<Tri> tris(sc.size() / 17);
    for (size_t i = 0; i < tris.size(); i++) {
        const double* r = &sc[17 * i];
        Tri& T = tris[i];
        T.v0 = V{r[0], r[1], r[2]};
        T.e1 = V{r[3], r[4], r[5]} - T.v0;
        T.e2 = V{r[6], r[7], r[8]} - T.v0;
        const V n = cross(T.e1, T.e2);
        T.n = dot(n, n) > 0.0 ? unit(n) : V{0.0, 0.0, 1.0}; /* a triangle without area is never hit */
        T.light = false;
        for (int k = 0; k < 3; k++) { T.albedo[k] = r[9 + k]; T.emission[k] = r[12 + k]; T.light = T.light || r[12 + k] > 0.0; }
        T.kind = (int)r[15];
        T.ior = r[16];
        if (T.kind < 0 || T.kind > 2 || (T.kind == 2 && !(T.ior >= 1.0))) { std::fprintf(stderr, "bad surface\n"); return 2; }
    }

    const int pixels = P.width * P.height, depths = P.bounces + 2;
    const size_t units = (size_t)P.batches * pixels;
    std::vector<double> sums(units * 6, 0.0), depth_sums(units * 3 * depths, 0.0);
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (;;) {
            const size_t u = next.fetch_add(1);
            if (u >= units) return;
            const int b = (int)(u / pixels), p = (int)(u % pixels);
            Rng g = keyed(P.seed, (uint64_t)b, (uint64_t)p);
            double* s = &sums[u * 6];
            double* by_depth = &depth_sums[u * 3 * depths];
            for (int i = 0; i < P.spp; i++) {
                double L[3];
                path(tris, P, p % P.width, p / P.width, g, L, by_depth);
                for (int k = 0; k < 3; k++) { s[k] += L[k]; s[3 + k] += L[k] * L[k]; }
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; t++) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();

    const int cw = P.width / P.cells_x, ch = P.height / P.cells_y, cells = P.cells_x * P.cells_y;
    std::vector<double> out(4 + 9 * cells + 9 + 3 * depths, 0.0);
    out[0] = (double)units * P.spp; out[1] = P.cells_y; out[2] = P.cells_x; out[3] = depths;
    for (int cy = 0; cy < P.cells_y; cy++)
        for (int cx = 0; cx < P.cells_x; cx++) {
            const Moments m = reduce(sums, P, cx * cw, (cx + 1) * cw, cy * ch, (cy + 1) * ch);
            const int c = cy * P.cells_x + cx;
            for (int k = 0; k < 3; k++) {
                out[4 + 3 * c + k] = m.mean[k];
                out[4 + 3 * cells + 3 * c + k] = m.se[k];
                out[4 + 6 * cells + 3 * c + k] = m.sd[k];
            }
        }
    const Moments f = reduce(sums, P, 0, P.width, 0, P.height);
    double* fo = &out[4 + 9 * cells];
    for (int k = 0; k < 3; k++) { fo[k] = f.mean[k]; fo[3 + k] = f.se[k]; fo[6 + k] = f.sd[k]; }
    for (size_t u = 0; u < units; u++)
        for (int j = 0; j < 3 * depths; j++) fo[9 + j] += depth_sums[u * 3 * depths + j];
    for (int j = 0; j < 3 * depths; j++) fo[9 + j] /= (double)units * P.spp;

    FILE* o = std::fopen(argv[3], "wb");
    if (!o || std::fwrite(out.data(), 8, out.size(), o) != out.size() || std::fclose(o) != 0) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 1; }
    std::printf("OK %.0f paths\n", out[0]);
    return 0;
}
