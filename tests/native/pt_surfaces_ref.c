/*
 * pt_surfaces_ref.c — test reference for path B's mirror and glass surfaces.
 *
 * TEST INFRASTRUCTURE ONLY: tests/test_pt_surfaces_ref.py compiles it with oracle B's arithmetic flags
 * (-O2 -ffp-contract=off -fno-fast-math -mfma) and links it against oracle/_build/liboracle.so.  Everything §6 already
 * defines comes from the oracle's exports (orb_closest_hit, orb_occluded, orb_rand, orb_cosine_dir); this file restates only
 * the camera ray (oracle_b.c:trace_path) and the path loop with surfaces.  With every triangle Lambert the loop is oracle B's,
 * operation for operation.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#include "../../oracle/oracle.h"

typedef struct { float x, y, z; } v3;
static inline v3 mk(float x, float y, float z) { v3 r = {x, y, z}; return r; }
static inline v3 sub(v3 a, v3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline v3 neg(v3 a) { return mk(-a.x, -a.y, -a.z); }
static inline v3 fma3(v3 a, float s, v3 b) { return mk(fmaf(a.x, s, b.x), fmaf(a.y, s, b.y), fmaf(a.z, s, b.z)); }
static inline float dot(v3 a, v3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
static inline v3 cross(v3 a, v3 b) {
    return mk(fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x)));
}
static inline v3 normalize(v3 a) {
    const float s = 1.0f / sqrtf(dot(a, a));
    return mk(a.x * s, a.y * s, a.z * s);
}
static inline v3 ld3(const float* p) { return mk(p[0], p[1], p[2]); }
static inline void st3(float* p, v3 a) { p[0] = a.x; p[1] = a.y; p[2] = a.z; }

typedef struct {
    orb_scene* s; /* oracle B's scene: closest hit and occlusion */
    uint32_t n, n_lights;
    float *v0, *e1, *e2, *albedo, *emission; /* original order */
    float* w;                                /* surface word: 0 Lambert, -1 mirror, eta glass */
    uint32_t* lights;                        /* emissive triangles, ascending */
} prs_scene;

void prs_scene_destroy(prs_scene* p) {
    if (!p) return;
    if (p->s) orb_scene_destroy(p->s);
    free(p->v0); free(p->e1); free(p->e2); free(p->albedo); free(p->emission); free(p->w); free(p->lights);
    free(p);
}

/* kind == NULL: all Lambert; ior is read where kind is 2 (glass) */
prs_scene* prs_scene_create(const float* verts, const float* albedo, const float* emission, const uint32_t* kind, const float* ior, uint32_t n) {
    if (!verts || !albedo || !emission || n == 0) return NULL;
    orb_mesh m = {n, verts, albedo, emission};
    prs_scene* p = (prs_scene*)calloc(1, sizeof *p);
    if (!p) return NULL;
    p->s = orb_scene_create(&m);
    p->n = n;
    p->v0 = malloc(12u * (size_t)n); p->e1 = malloc(12u * (size_t)n); p->e2 = malloc(12u * (size_t)n);
    p->albedo = malloc(12u * (size_t)n); p->emission = malloc(12u * (size_t)n);
    p->w = malloc(4u * (size_t)n); p->lights = malloc(4u * (size_t)n);
    if (!p->s || !p->v0 || !p->e1 || !p->e2 || !p->albedo || !p->emission || !p->w || !p->lights) {
        prs_scene_destroy(p);
        return NULL;
    }
    for (uint32_t i = 0; i < n; i++) {
        const float* v = verts + 9 * (size_t)i;
        for (int a = 0; a < 3; a++) {
            p->v0[3 * i + a] = v[a];
            p->e1[3 * i + a] = v[3 + a] - v[a]; /* spec §6.1: edges are formed once, in fp32 */
            p->e2[3 * i + a] = v[6 + a] - v[a];
        }
        const float* e = emission + 3 * (size_t)i;
        if (e[0] > 0.0f || e[1] > 0.0f || e[2] > 0.0f) p->lights[p->n_lights++] = i;
        p->w[i] = !kind ? 0.0f : kind[i] == 1u ? -1.0f : kind[i] == 2u ? ior[i] : 0.0f;
    }
    memcpy(p->albedo, albedo, 12u * (size_t)n);
    memcpy(p->emission, emission, 12u * (size_t)n);
    return p;
}

/* ---- spec §6.11: Fresnel reflectance and the continuation at a mirror / glass vertex ------------------------------------ */
/* c = cos(incidence) >= 0, eta = relative index n_from / n_to; 1 for total internal reflection.  *ct_out = cos(transmission) */
static inline float fresnel(float c, float eta, float* ct_out) {
    const float s2 = (eta * eta) * fmaf(-c, c, 1.0f);
    *ct_out = 0.0f;
    if (!(s2 < 1.0f)) return 1.0f;
    const float ct = sqrtf(1.0f - s2);
    const float a = eta * c, b = eta * ct;
    const float rs = (a - ct) / (a + ct), rp = (c - b) / (c + b);
    *ct_out = ct;
    return fmaf(rs, rs, rp * rp) * 0.5f;
}

/* w < 0 mirror, w >= 1 glass; n faces the incoming ray d (flipped: it had to be turned, the ray leaves the glass) */
static inline v3 delta_dir(v3 d, v3 n, float w, int flipped, float u, int* below) {
    const float c = -dot(n, d);
    *below = 0;
    if (w > 0.0f) {
        const float eta = flipped ? w : 1.0f / w;
        float ct;
        const float F = fresnel(c, eta, &ct);
        if (!(u < F)) {
            *below = 1;
            const float k = eta * c - ct;
            return mk(fmaf(n.x, k, eta * d.x), fmaf(n.y, k, eta * d.y), fmaf(n.z, k, eta * d.z));
        }
    }
    return fma3(n, c + c, d);
}

float prs_fresnel(float c, float eta) {
    float ct;
    return fresnel(c, eta, &ct);
}
void prs_delta_dir(const float d[3], const float n[3], float w, int flipped, float u, float out[3], int* below) {
    st3(out, delta_dir(ld3(d), ld3(n), w, flipped, u, below));
}

/* ---- the camera ray: oracle_b.c:trace_path ------------------------------------------------------------------------------- */
static inline v3 rotate_q(const float q[4], v3 v) { /* shaders/utilities.glsl:26-29 */
    v3 qv = mk(q[0], q[1], q[2]);
    v3 c = cross(qv, v);
    v3 t = mk(fmaf(q[3], v.x, c.x), fmaf(q[3], v.y, c.y), fmaf(q[3], v.z, c.z));
    v3 c2 = cross(qv, t);
    return mk(fmaf(2.0f, c2.x, v.x), fmaf(2.0f, c2.y, v.y), fmaf(2.0f, c2.z, v.z));
}

/* ---- spec §6.4 + §6.11: one path ----------------------------------------------------------------------------------------- */
static void trace_path(const prs_scene* ps, const orb_params* p, uint32_t px, uint32_t py, uint32_t sample, float L[3], uint64_t ct[3]) {
    const uint32_t pix = py * p->width + px;
    const float nx = ((((float)px + orb_rand(pix, sample, 0, 0, p->seed)) * 2.0f) / (float)p->width - 1.0f) * p->ratio[0];
    const float ny = ((((float)py + orb_rand(pix, sample, 0, 1, p->seed)) * 2.0f) / (float)p->height - 1.0f) * p->ratio[1];
    v3 d = normalize(rotate_q(p->rot, mk(nx, 1.0f, ny)));
    v3 o = ld3(p->pos);
    float T[3] = {1.0f, 1.0f, 1.0f};
    int after_delta = 0; /* the previous vertex was a mirror or glass vertex */
    L[0] = L[1] = L[2] = 0.0f;
    for (uint32_t depth = 0;; depth++) {
        ct[depth == 0 ? 0 : 1]++;
        float of[3], df[3], t;
        st3(of, o);
        st3(df, d);
        const int32_t tri = orb_closest_hit(ps->s, of, df, &t, 1);
        if (tri < 0) { /* left the scene */
            for (int k = 0; k < 3; k++) L[k] = fmaf(T[k], p->sky[k], L[k]);
            break;
        }
        const float* em = ps->emission + 3 * (size_t)tri;
        if (em[0] > 0.0f || em[1] > 0.0f || em[2] > 0.0f) { /* camera rays and rays leaving a delta vertex see lights */
            if (depth == 0 || after_delta)
                for (int k = 0; k < 3; k++) L[k] = fmaf(T[k], em[k], L[k]);
            break;
        }
        const float* alb = ps->albedo + 3 * (size_t)tri;
        const float w = ps->w[tri];
        v3 n = normalize(cross(ld3(ps->e1 + 3 * (size_t)tri), ld3(ps->e2 + 3 * (size_t)tri)));
        const int flipped = dot(n, d) > 0.0f;
        if (flipped) n = neg(n);
        const v3 pt = fma3(d, t, o);
        const v3 po = fma3(n, p->ray_eps, pt);
        if (w != 0.0f) { /* mirror or glass: no next-event estimation */
            if (depth >= p->bounces) break;
            int below;
            d = delta_dir(d, n, w, flipped, orb_rand(pix, sample, depth, 7, p->seed), &below);
            o = below ? fma3(n, -p->ray_eps, pt) : po;
            for (int k = 0; k < 3; k++) T[k] *= alb[k];
            after_delta = 1;
            continue;
        }
        after_delta = 0;
        if (ps->n_lights > 0) { /* next-event estimation, oracle_b.c:trace_path */
            uint32_t k = (uint32_t)(orb_rand(pix, sample, depth, 2, p->seed) * (float)ps->n_lights);
            if (k > ps->n_lights - 1) k = ps->n_lights - 1;
            const uint32_t lt = ps->lights[k];
            const float su = sqrtf(orb_rand(pix, sample, depth, 3, p->seed)), u2 = orb_rand(pix, sample, depth, 4, p->seed);
            const float b1 = su * (1.0f - u2), b2 = su * u2;
            const v3 lv0 = ld3(ps->v0 + 3 * (size_t)lt), le1 = ld3(ps->e1 + 3 * (size_t)lt), le2 = ld3(ps->e2 + 3 * (size_t)lt);
            const v3 q = mk(fmaf(le2.x, b2, fmaf(le1.x, b1, lv0.x)), fmaf(le2.y, b2, fmaf(le1.y, b1, lv0.y)), fmaf(le2.z, b2, fmaf(le1.z, b1, lv0.z)));
            const v3 wi = sub(q, po);
            const float d2 = dot(wi, wi);
            const v3 nl = cross(le1, le2);
            const float cs = dot(n, wi), cl = fabsf(dot(nl, wi));
            const float d4 = d2 * d2; /* oracle_b.c: 0 for a light closer than about 2^-37 */
            if (cs > 0.0f && cl > 0.0f && d4 > 0.0f) {
                const float wt = ((cs * cl) * ((float)ps->n_lights * 0.15915494f)) / d4;
                const float* le = ps->emission + 3 * (size_t)lt;
                float c3[3];
                for (int j = 0; j < 3; j++) c3[j] = ((T[j] * alb[j]) * le[j]) * wt;
                float pf[3], wf[3];
                st3(pf, po);
                st3(wf, wi);
                ct[2]++;
                if (!orb_occluded(ps->s, pf, wf, 1))
                    for (int j = 0; j < 3; j++) L[j] += c3[j];
            }
        }
        if (depth >= p->bounces) break;
        float nf[3], nd[3];
        st3(nf, n);
        orb_cosine_dir(nf, orb_rand(pix, sample, depth, 5, p->seed), orb_rand(pix, sample, depth, 6, p->seed), nd);
        d = ld3(nd);
        o = po;
        for (int k = 0; k < 3; k++) T[k] *= alb[k];
    }
}

/* rows [row0, row1) of the frame (rgb holds (row1-row0)*width*3 floats), as orb_render_rows; counts = camera, bounce, shadow rays */
int prs_render_rows(const prs_scene* ps, const orb_params* p, uint32_t row0, uint32_t row1, float* rgb, uint64_t counts[3], int threads) {
    if (!ps || !p || !rgb || p->width == 0 || p->height == 0 || p->spp == 0 || row0 >= row1 || row1 > p->height) return -1;
#ifdef _OPENMP
    if (threads <= 0) threads = omp_get_max_threads();
#else
    threads = 1;
#endif
    uint64_t cam = 0, bnc = 0, shd = 0;
#pragma omp parallel for schedule(dynamic, 2) num_threads(threads) reduction(+ : cam, bnc, shd)
    for (uint32_t py = row0; py < row1; py++) {
        uint64_t ct[3] = {0, 0, 0};
        for (uint32_t px = 0; px < p->width; px++) {
            float acc[3] = {0.0f, 0.0f, 0.0f};
            for (uint32_t s = 0; s < p->spp; s++) { /* spec §6.6: samples are summed in index order */
                float L[3];
                trace_path(ps, p, px, py, s, L, ct);
                acc[0] += L[0]; acc[1] += L[1]; acc[2] += L[2];
            }
            float* o = rgb + ((size_t)(py - row0) * p->width + px) * 3;
            o[0] = acc[0] / (float)p->spp; o[1] = acc[1] / (float)p->spp; o[2] = acc[2] / (float)p->spp;
        }
        cam += ct[0]; bnc += ct[1]; shd += ct[2];
    }
    if (counts) { counts[0] = cam; counts[1] = bnc; counts[2] = shd; }
    return 0;
}
