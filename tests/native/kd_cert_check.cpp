// kd_cert_check.cpp — the T* certificate (csrc/bvh_common.h rt_kd_cert) checked on the
// library's own prepared arrays, ray by ray, against the plain KD traversal:
//
//  * tables: every safe box has the final-pass property (every KD leaf whose closed cell meets it lists
//    the slot's triangle — an independent recursive sweep, not scene_prepare's), every split value is a
//    member of its axis' hash set, the load factor is <= 0.5 (shipped: <= 0.25), and -0 finds +0;
//  * rays: the bounded traversal as the kernels run it — the s_min query, then the certificate, then
//    (uncertified) the bounded KD descent — returns the plain KD traversal's triangle and barycentrics
//    bit for bit; a certified ray's descent is run too and must agree;
//  * slack: for every ray whose hit point passes the box test, the shipped delta (rt_cert_delta) is at
//    least 4x the derived bound e_P + delta_desc + the box comparison's own rounding, evaluated from
//    the ray's actual magnitudes in double.
//
// Ray sets: the mix of wide_smin_check.cpp (camera rays, bounces off random triangles — some grazing,
// some axis-parallel —, chords of transparent objects), rays whose origin coordinate IS a split value
// on an axis they go up / down (the reference's H5 quirk: t = 0 goes to the lower side), and rays aimed
// at the extreme vertex of a triangle on a random axis (the hit point closest to a safe-box face).
//
// Two more ray sets have modes of their own:
//  * `file`: rays read from a raw float32 (n, 6) file {o, d} — the oracle's own camera, extension and shadow rays
//    of path-traced pixels (or_log_rays, as tools/dump_rays.py writes them): real bounce origins are computed
//    hit points lying off their triangle, and the directions are the shading's;
//  * `faces`: rays built from the safe-box table so that the hit point X lands ON the certificate's box
//    threshold.  For a slot and a face (axis a, side) whose threshold plane x_a = lo_a + delta (hi_a - delta)
//    cuts the triangle, a point Q of the triangle on that plane, moved by -4..4 ulp across it, is aimed at from
//    a nearby origin; rays whose computed X_a is within 8 ulp of the threshold on the slot they were aimed at
//    are counted, with how many certified and how many fell back as RT_CERT_BOX.  Both must occur.
//
// usage: kd_cert_check scene.txt [rays] [seed] ["x y z" camera position, hex floats]
//        kd_cert_check scene.txt file rays.f32
//        kd_cert_check scene.txt faces [rays] [seed]
// prints "certified C of H hits (share S)" and the fallback reasons; exit 0 = all identical.
#include <math.h>
#include <omp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "bvh_common.h"
#include "host/bvh_build.h"
#include "host/rt_host.h"

namespace {

float bitsf(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}
uint32_t fbits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

struct Hit {
    int tri = -1;
    float b[3] = {0, 0, 0};
};

bool scene_box(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float &t1, float &t2)
{
    const Bounding_Box &b = h.bounds;
    float tminx = (b.min.x - o.x) / d.x, tminy = (b.min.y - o.y) / d.y, tminz = (b.min.z - o.z) / d.z;
    float tmaxx = (b.max.x - o.x) / d.x, tmaxy = (b.max.y - o.y) / d.y, tmaxz = (b.max.z - o.z) / d.z;
    t1 = fmaxf(fmaxf(fminf(tminx, tmaxx), fminf(tminy, tmaxy)), fminf(tminz, tmaxz));
    t2 = fminf(fminf(fmaxf(tminx, tmaxx), fmaxf(tminy, tmaxy)), fmaxf(tminz, tmaxz));
    return t1 <= t2;
}

// bvh_trace.h kd_bounded (s_min = -inf: trace_ray itself); tstar >= 0: a leaf listing T* tests its entry alone
Hit kd_trace(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float entry, float exit_, float s_min, int tstar)
{
    Hit hit;
    struct E { uint32_t node; float entry; } stk[64];
    int sp = 0;
    const float root_exit = exit_;
    uint32_t node = 0;
    while (true) {
        uint32_t nx = h.nodes[2 * node], ny = h.nodes[2 * node + 1];
        while ((ny & 3u) != RT_LEAF_TAG) {
            const uint32_t axis = ny & 3u;
            const float split = bitsf(nx);
            const float oax = axis == 0 ? o.x : (axis == 1 ? o.y : o.z);
            const float dax = axis == 0 ? d.x : (axis == 1 ? d.y : d.z);
            uint32_t near_c = node + 1, far_c = ny >> 2;
            if (oax >= split) std::swap(near_c, far_c);
            const float t = (split - oax) / dax;
            if (t >= exit_ || t < 0) {
                node = near_c;
            } else if (t <= entry) {
                node = far_c;
            } else if (t <= s_min) {
                node = far_c;
                entry = t;
            } else {
                stk[sp++] = E{far_c, t};
                node = near_c;
                exit_ = t;
            }
            nx = h.nodes[2 * node];
            ny = h.nodes[2 * node + 1];
        }
        const uint32_t count = ny >> 2;
        if (count > 0 && exit_ > s_min) {
            float smallest = exit_;
            uint32_t lo = nx, hi = nx + count;
            if (tstar >= 0)
                for (uint32_t e = nx; e < nx + count; ++e)
                    if (h.isect_tri[e] == (uint32_t)tstar) {
                        lo = e;
                        hi = e + 1;
                        break;
                    }
            for (uint32_t e = lo; e < hi; ++e) {
                float s, b[3];
                if (rt_tri_plane(h.isect_a[e], o, d, smallest, s) &&
                    rt_tri_bary(h.isect_bary[e].b, h.isect_bary[e].c, h.isect_bary[e].d, bitsf(h.isect_bary[e].rd), o, d,
                                s, b[0], b[1], b[2])) {
                    smallest = s;
                    hit.tri = (int)h.isect_bary[e].tri;
                    memcpy(hit.b, b, sizeof b);
                }
            }
            if (hit.tri >= 0) return hit;
            if (hi - lo != count) {
                fprintf(stderr, "T* entry of a leaf did not pass\n");
                exit(3);
            }
        }
        if (sp == 0) return hit;
        --sp;
        node = stk[sp].node;
        entry = stk[sp].entry;
        exit_ = sp > 0 ? stk[sp - 1].entry : root_exit;
    }
}

// the s_min query (bvh_trace.h bvh4_query): nearest child first, best lowered test by test; tk as leaf_scan_min
float seq_query(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float best, int &tk)
{
    tk = -1;
    const RtSlab sl = rt_slab(o, d, rt_ray_margin(o.x, o.y, o.z, h.bvh_scale));
    struct E { uint32_t ref; float tn; };
    std::vector<E> stk;
    uint32_t cur = 0;
    auto pop = [&]() -> uint32_t {
        while (!stk.empty()) {
            const E e = stk.back();
            stk.pop_back();
            if (e.tn <= best) return e.ref;
        }
        return RT_BVH_EMPTY;
    };
    while (true) {
        while (!(cur & RT_BVH_LEAF)) {
            const float *f = reinterpret_cast<const float *>(&h.bvh4[8 * (size_t)cur]);
            const uint32_t *rf = reinterpret_cast<const uint32_t *>(f + 24);
            E c[4];
            for (int k = 0; k < 4; ++k) {
                float tn;
                const bool hit = rt_bvh_box(f[k], f[4 + k], f[8 + k], f[12 + k], f[16 + k], f[20 + k], sl, best, tn) &&
                                 rf[k] != RT_BVH_EMPTY;
                c[k] = hit ? E{rf[k], tn} : E{RT_BVH_EMPTY, INFINITY};
            }
            std::stable_sort(c, c + 4, [](const E &a, const E &b) {
                const bool ea = a.ref == RT_BVH_EMPTY, eb = b.ref == RT_BVH_EMPTY;
                return ea != eb ? eb : a.tn < b.tn;
            });
            for (int k = 3; k >= 1; --k)
                if (c[k].ref != RT_BVH_EMPTY) stk.push_back(c[k]);
            cur = c[0].ref != RT_BVH_EMPTY ? c[0].ref : pop();
        }
        if (cur == RT_BVH_EMPTY) break;
        const uint32_t first = (cur & ~RT_BVH_LEAF) >> 3, end = first + (cur & 7u) + 1u;
        for (uint32_t e = first; e < end; ++e) {
            float s, b[3];
            if (!rt_tri_plane(h.bvh_a[e], o, d, INFINITY, s) || !(s <= best)) continue;
            const bool lt = s < best;
            if (!lt && tk < 0) continue;
            const RtIsectBary &R = h.bvh_bary[e];
            if (!rt_tri_bary(R.b, R.c, R.d, bitsf(R.rd), o, d, s, b[0], b[1], b[2])) continue;
            if (lt) {
                best = s;
                tk = (int)e;
            } else {
                tk = -2; // RT_TK_TIE
            }
        }
        cur = pop();
        if (cur == RT_BVH_EMPTY) break;
    }
    return best;
}

// ---- the tables
// leaves whose closed cell meets [blo, bhi] and that do not list triangle t (recursive, on its own)
long long leaves_without(const rt_host::PreparedHost &h, uint32_t node, const float *clo, const float *chi,
                         const float *blo, const float *bhi, uint32_t t)
{
    for (int a = 0; a < 3; ++a)
        if (!(std::max(clo[a], blo[a]) <= std::min(chi[a], bhi[a]))) return 0;
    const uint32_t x = h.nodes[2 * (size_t)node], y = h.nodes[2 * (size_t)node + 1];
    if ((y & 3u) == RT_LEAF_TAG) {
        for (uint32_t e = x; e < x + (y >> 2); ++e)
            if (h.isect_tri[e] == t) return 0;
        return 1;
    }
    const int a = (int)(y & 3u);
    const float split = bitsf(x);
    float lhi[3] = {chi[0], chi[1], chi[2]}, rlo[3] = {clo[0], clo[1], clo[2]};
    lhi[a] = std::min(lhi[a], split);
    rlo[a] = std::max(rlo[a], split);
    return leaves_without(h, node + 1, clo, lhi, blo, bhi, t) + leaves_without(h, y >> 2, rlo, chi, blo, bhi, t);
}

int check_tables(const rt_host::PreparedHost &h, long long &nonempty)
{
    const size_t ns = h.bvh_bary.size();
    if (h.kd_safe.size() != 2 * ns) return 1;
    long long bad = 0, ne = 0;
#pragma omp parallel for schedule(dynamic, 1024) reduction(+ : bad, ne)
    for (long long k = 0; k < (long long)ns; ++k) {
        const RtF4 lo = h.kd_safe[2 * (size_t)k], hi = h.kd_safe[2 * (size_t)k + 1];
        if (!(lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z)) continue;
        ++ne;
        const float blo[3] = {lo.x, lo.y, lo.z}, bhi[3] = {hi.x, hi.y, hi.z};
        const float clo[3] = {-INFINITY, -INFINITY, -INFINITY}, chi[3] = {INFINITY, INFINITY, INFINITY};
        bad += leaves_without(h, 0, clo, chi, blo, bhi, h.bvh_bary[(size_t)k].tri);
    }
    nonempty = ne;
    if (bad) return 2;
    const RtKdCert kc = h.kd_cert();
    for (int a = 0; a < 3; ++a) {
        const size_t n = (size_t)(h.split_off[a + 1] - h.split_off[a]), size = (size_t)1 << (32 - h.split_hshift[a]);
        if (2 * n > size) return 3; // load factor
        size_t used = 0;
        for (size_t i = 0; i < size; ++i) used += h.split_hash[(size_t)h.split_hoff[a] + i] != RT_SPLIT_EMPTY;
        if (used > n) return 4;
        for (size_t k = 0; k < n; ++k) {
            const float v = h.split_vals[(size_t)h.split_off[a] + k];
            if (!rt_split_member(kc.hash + kc.hoff[a], kc.hshift[a], v)) return 5;
            if (v == 0.0f && !rt_split_member(kc.hash + kc.hoff[a], kc.hshift[a], -v)) return 6;
        }
    }
    return 0;
}

struct Tally {
    long long rays = 0, bounded = 0, hits = 0, certified = 0, mism = 0, cert_descent_mism = 0, slack_bad = 0,
              reason[6] = {0, 0, 0, 0, 0, 0}, on_split_up = 0, on_split_up_cert = 0, face_near = 0, face_cert = 0,
              face_box = 0;
    double min_ratio = INFINITY;
    void add(const Tally &o)
    {
        rays += o.rays; bounded += o.bounded; hits += o.hits; certified += o.certified; mism += o.mism;
        cert_descent_mism += o.cert_descent_mism; slack_bad += o.slack_bad;
        on_split_up += o.on_split_up; on_split_up_cert += o.on_split_up_cert;
        face_near += o.face_near; face_cert += o.face_cert; face_box += o.face_box;
        for (int k = 0; k < 6; ++k) reason[k] += o.reason[k];
        min_ratio = std::min(min_ratio, o.min_ratio);
    }
};

bool same(const Hit &a, const Hit &b) { return a.tri == b.tri && memcmp(a.b, b.b, sizeof a.b) == 0; }

struct Last { // what the certificate said about the last ray (why < 0: it was never asked)
    int why = -1, tk = -1;
    float s_min = 0.0f;
};

void check_ray(const rt_host::PreparedHost &h, const RtKdCert &kc, Vec3D o, Vec3D d, Tally &t, Last *last = nullptr)
{
    if (last) *last = Last{};
    float t1, t2;
    if (!scene_box(h, o, d, t1, t2)) return;
    if (!rt_bounded_ray(o, d, h.split_vals.data(), h.split_off)) return;
    ++t.bounded;
    const Hit plain = kd_trace(h, o, d, t1, t2, -INFINITY, -1);
    if (plain.tri >= 0) ++t.hits;
    int tk;
    const float s_min = seq_query(h, o, d, t2, tk);
    Hit got;
    if (s_min < t2) { // (else: a miss, as trace_bvh returns it)
        const int why = rt_kd_cert(kc, o, d, t1, t2, s_min, tk);
        ++t.reason[why];
        if (last) *last = Last{why, tk, s_min};
        const float *oa = &o.x, *da = &d.x;
        bool up_on_split = false;
        for (int a = 0; a < 3; ++a)
            up_on_split = up_on_split || (da[a] > 0.0f && rt_sorted_contains(h.split_vals.data(), h.split_off[a],
                                                                              h.split_off[a + 1], oa[a]));
        if (up_on_split) {
            ++t.on_split_up;
            if (why == RT_CERT_OK) ++t.on_split_up_cert; // (must stay 0: the hash sets' job)
        }
        const Hit desc = kd_trace(h, o, d, t1, t2, s_min, tk >= 0 ? (int)h.bvh_bary[tk].tri : -1);
        if (why == RT_CERT_OK) {
            ++t.certified;
            const RtIsectBary &R = h.bvh_bary[tk];
            if (rt_tri_bary(R.b, R.c, R.d, bitsf(R.rd), o, d, s_min, got.b[0], got.b[1], got.b[2])) got.tri = (int)R.tri;
            if (!same(got, desc)) ++t.cert_descent_mism;
        } else {
            got = desc;
        }
        // the slack, wherever the box test passes (the certificate relies on delta only there)
        if (tk >= 0 && (why == RT_CERT_OK || why == RT_CERT_ORIGIN)) {
            const double u = 0x1p-24, dl = rt_cert_delta(o, kc.scale);
            const float X[3] = {o.x + d.x * s_min, o.y + d.y * s_min, o.z + d.z * s_min};
            for (int a = 0; a < 3; ++a) {
                const double ax = fabs((double)X[a]), ao = fabs((double)oa[a]);
                const double eP = u * (2.0 * ax + ao) * (1.0 + 0x1p-20) + 0x1p-140;
                const double ddesc = (2.0 * u + u * u) * (ax + dl + ao);
                const double cmp = u * (ax + 2.0 * dl);
                const double need = eP + ddesc + cmp;
                t.min_ratio = std::min(t.min_ratio, dl / need);
                if (!(dl >= 4.0 * need)) ++t.slack_bad;
            }
        }
    }
    if (!same(got, plain)) {
        if (++t.mism <= 3)
            fprintf(stderr, "MISMATCH o (%a %a %a) d (%a %a %a): kd %d, certificate path %d (tk %d)\n", o.x, o.y, o.z, d.x,
                    d.y, d.z, plain.tri, got.tri, tk);
    }
}

int report(const Tally &t)
{
    printf("rays %lld bounded %lld hits %lld\n", t.rays, t.bounded, t.hits);
    printf("mismatches %lld certified-vs-descent mismatches %lld slack violations %lld split-origin certified %lld\n",
           t.mism, t.cert_descent_mism, t.slack_bad, t.on_split_up_cert);
    printf("certified %lld of %lld hits share %.6f\n", t.certified, t.hits, t.hits ? (double)t.certified / t.hits : 0.0);
    printf("fallbacks: tie %lld interval %lld direction %lld origin %lld box %lld; split-origin rays going up %lld\n",
           t.reason[RT_CERT_TIE], t.reason[RT_CERT_INTERVAL], t.reason[RT_CERT_DIR], t.reason[RT_CERT_ORIGIN],
           t.reason[RT_CERT_BOX], t.on_split_up);
    printf("smallest delta / derived bound %.3f\n", t.min_ratio);
    return t.mism == 0 && t.cert_descent_mism == 0 && t.slack_bad == 0 && t.on_split_up_cert == 0 ? 0 : 1;
}

// `file`: the rays of a raw float32 (n, 6) file
int run_file(const rt_host::PreparedHost &h, const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    std::vector<float> v;
    float buf[6 * 4096];
    size_t got;
    while ((got = fread(buf, sizeof(float), 6 * 4096, f)) > 0) v.insert(v.end(), buf, buf + got);
    fclose(f);
    const long long n = (long long)(v.size() / 6);
    const RtKdCert kc = h.kd_cert();
    Tally total;
#pragma omp parallel
    {
        Tally t;
#pragma omp for schedule(dynamic, 1024)
        for (long long k = 0; k < n; ++k) {
            const float *r = &v[6 * (size_t)k];
            ++t.rays;
            check_ray(h, kc, rt_v3(r[0], r[1], r[2]), rt_v3(r[3], r[4], r[5]), t);
        }
#pragma omp critical
        total.add(t);
    }
    return report(total);
}

// `faces`: rays whose hit point lands on a safe box's threshold plane (see the head comment)
int run_faces(const rt_host::PreparedHost &h, const RtHostScene &scene, long long rays, unsigned long long seed)
{
    const RtKdCert kc = h.kd_cert();
    const size_t ns = h.bvh_bary.size();
    Tally total;
#pragma omp parallel
    {
        Tally t;
        std::mt19937_64 rng(seed + 0x9e3779b97f4a7c15ull * (unsigned)(omp_get_thread_num() + 1));
        std::uniform_real_distribution<float> U(0.0f, 1.0f);
#pragma omp for schedule(dynamic, 256)
        for (long long k = 0; k < rays; ++k) {
            bool made = false;
            Vec3D o = rt_v3(0, 0, 0), d = rt_v3(0, 0, 0);
            int slot = -1, axis = 0;
            float thr = 0.0f;
            for (int attempt = 0; attempt < 64 && !made; ++attempt) {
                slot = (int)((size_t)(U(rng) * ns) % ns);
                const RtF4 lo = h.kd_safe[2 * (size_t)slot], hi = h.kd_safe[2 * (size_t)slot + 1];
                if (!(lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z)) continue;
                const Triangle &tr = scene.tris[h.bvh_bary[(size_t)slot].tri];
                const Vec3D p[3] = {tr.p1, tr.p2, tr.p3};
                Vec3D nn = rt_normalize(rt_cross(tr.p2 - tr.p1, tr.p3 - tr.p1));
                if (nn.x != nn.x) continue;
                // the offset from the hit point to the origin: off the triangle's plane, a small part of the scene
                Vec3D v = rt_v3(2 * U(rng) - 1, 2 * U(rng) - 1, 2 * U(rng) - 1);
                if (rt_dot(v, nn) < 0) v = -v;
                v = (0.002f + 0.05f * U(rng)) * (h.bvh_scale + 1e-3f) * rt_normalize(rt_normalize(v) + 0.3f * nn);
                if (v.x != v.x) continue;
                const int face0 = (int)(U(rng) * 6) % 6;
                for (int fc = 0; fc < 6 && !made; ++fc) {
                    const int face = (face0 + fc) % 6;
                    axis = face % 3;
                    const bool upper = face >= 3;
                    const float bound = upper ? (&hi.x)[axis] : (&lo.x)[axis];
                    Vec3D Q = (1.0f / 3.0f) * (p[0] + p[1] + p[2]);
                    bool ok = true;
                    for (int it = 0; it < 2 && ok; ++it) { // (delta depends on the origin Q + v: settle it)
                        const float dl = rt_cert_delta(Q + v, kc.scale);
                        thr = upper ? bound - dl : bound + dl;
                        Vec3D e[3];
                        int ne = 0;
                        for (int i = 0; i < 3; ++i) {
                            const Vec3D &a0 = p[i], &a1 = p[(i + 1) % 3];
                            const float c0 = (&a0.x)[axis], c1 = (&a1.x)[axis];
                            if (c0 == c1 || (c0 - thr) * (c1 - thr) > 0) continue;
                            e[ne++] = a0 + ((thr - c0) / (c1 - c0)) * (a1 - a0);
                        }
                        if (ne < 2) {
                            ok = false;
                            break;
                        }
                        const float w = 0.15f + 0.7f * U(rng);
                        Q = e[0] + w * (e[1] - e[0]);
                    }
                    if (!ok) continue;
                    // -4 .. 4 ulp across the threshold on that axis
                    float c = thr;
                    const int j = (int)(U(rng) * 9) % 9 - 4;
                    for (int q = 0; q < (j < 0 ? -j : j); ++q) c = nextafterf(c, j < 0 ? -INFINITY : INFINITY);
                    (&Q.x)[axis] = c;
                    o = Q + v;
                    d = rt_normalize(Q - o);
                    made = d.x == d.x;
                }
            }
            ++t.rays;
            if (!made) continue;
            Last last;
            check_ray(h, kc, o, d, t, &last);
            if (last.why < 0 || last.tk != slot || (last.why != RT_CERT_OK && last.why != RT_CERT_BOX)) continue;
            // the threshold as rt_kd_cert evaluates it for this ray, and X_a's distance from it in ulp
            const RtF4 lo = h.kd_safe[2 * (size_t)slot], hi = h.kd_safe[2 * (size_t)slot + 1];
            const float dl = rt_cert_delta(o, kc.scale);
            const float X = (&o.x)[axis] + (&d.x)[axis] * last.s_min;
            const float tl = (&lo.x)[axis] + dl, th = (&hi.x)[axis] - dl;
            const float near_t = fabsf(X - tl) < fabsf(X - th) ? tl : th;
            const float ulp = nextafterf(fabsf(near_t), INFINITY) - fabsf(near_t);
            if (fabsf(X - near_t) <= 8.0f * ulp) {
                ++t.face_near;
                if (last.why == RT_CERT_OK) ++t.face_cert;
                else ++t.face_box;
            }
        }
#pragma omp critical
        total.add(t);
    }
    const int rc = report(total);
    printf("face rays within 8 ulp of a box threshold %lld certified %lld box-fallback %lld\n", total.face_near,
           total.face_cert, total.face_box);
    return rc != 0 ? rc : (total.face_cert > 0 && total.face_box > 0 ? 0 : 1);
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: %s scene.txt [rays] [seed] [camera]\n", argv[0]);
        return 2;
    }
    RtHostScene scene;
    Camera cam;
    if (rt_host::load_scene_file(scene, argv[1], &cam) != RT_OK) {
        fprintf(stderr, "scene load failed\n");
        return 2;
    }
    const int n = (int)scene.tris.size();
    std::vector<KD_Tree_Node> nodes;
    std::vector<int> indices;
    Bounding_Box bounds;
    if (rt_host::build_kd_tree(scene.tris.data(), n, nodes, indices, bounds) != RT_OK) return 2;
    std::vector<int> lights = rt_host::light_list(scene.tris.data(), n);
    rt_host::PreparedHost h;
    const double t0 = omp_get_wtime();
    if (rt_host::prepare_host(scene.tris.data(), n, nodes.data(), (int)nodes.size(), indices.data(),
                              (int)indices.size(), lights.data(), (int)lights.size(), bounds, h) != RT_OK ||
        h.bvh_depth < 0 || h.kd_safe.empty()) {
        fprintf(stderr, "prepare failed / no BVH or certificate tables built\n");
        return 2;
    }
    const double t_prep = omp_get_wtime() - t0;
    long long nonempty = 0;
    const int tc = check_tables(h, nonempty);
    printf("tris %d slots %zu safe boxes %lld prepare %.3f s cert bytes %zu tables %d\n", n, h.bvh_bary.size(), nonempty,
           t_prep, h.kd_safe.size() * sizeof(RtF4) + h.split_hash.size() * 4, tc);
    if (tc != 0) return 1;
    if (argc > 3 && strcmp(argv[2], "file") == 0) return run_file(h, argv[3]);
    if (argc > 2 && strcmp(argv[2], "faces") == 0)
        return run_faces(h, scene, argc > 3 ? atoll(argv[3]) : 200000, argc > 4 ? strtoull(argv[4], nullptr, 10) : 7);

    const long long rays = argc > 2 ? atoll(argv[2]) : 200000;
    const unsigned long long seed = argc > 3 ? strtoull(argv[3], nullptr, 10) : 7;
    if (argc > 4 && sscanf(argv[4], "%a %a %a", &cam.position.x, &cam.position.y, &cam.position.z) != 3) {
        fprintf(stderr, "bad camera position '%s'\n", argv[4]);
        return 2;
    }
    std::vector<int> glass;
    for (int i = 0; i < n; ++i)
        if (scene.tris[(size_t)i].material.transparent) glass.push_back(i);
    const RtKdCert kc = h.kd_cert();
    Tally total;
#pragma omp parallel
    {
        Tally t;
        std::mt19937_64 rng(seed + 0x9e3779b97f4a7c15ull * (unsigned)(omp_get_thread_num() + 1));
        std::uniform_real_distribution<float> U(0.0f, 1.0f);
        auto unit = [&]() {
            while (true) {
                Vec3D v = rt_v3(2 * U(rng) - 1, 2 * U(rng) - 1, 2 * U(rng) - 1);
                const float l = rt_dot(v, v);
                if (l > 1e-6f && l <= 1.0f) return rt_normalize(v);
            }
        };
        auto on_tri = [&](const Triangle &tr) {
            float b1 = U(rng), b2 = U(rng);
            if (b1 + b2 > 1) {
                b1 = 1 - b1;
                b2 = 1 - b2;
            }
            return tr.p1 + b1 * (tr.p2 - tr.p1) + b2 * (tr.p3 - tr.p1);
        };
        auto rand_tri = [&]() -> const Triangle & { return scene.tris[(size_t)(U(rng) * n) % n]; };
#pragma omp for schedule(dynamic, 1024)
        for (long long k = 0; k < rays; ++k) {
            Vec3D o, d;
            const int mode = (int)(k % 8);
            if (mode == 0) { // from the camera
                o = cam.position;
                d = unit();
            } else if (mode == 6) {
                // an origin coordinate that IS a split value, the ray going up (k & 8) or down that axis
                const int a = (int)(k >> 4) % 3;
                const int ns = h.split_off[a + 1] - h.split_off[a];
                o = on_tri(rand_tri());
                d = unit();
                if (ns > 0) {
                    const float v = h.split_vals[(size_t)h.split_off[a] + (size_t)(U(rng) * ns) % ns];
                    float *oa = &o.x, *da = &d.x;
                    oa[a] = v;
                    da[a] = (k & 8) ? fabsf(da[a]) : -fabsf(da[a]);
                }
            } else if (mode == 7) {
                // aimed just inside a triangle's extreme vertex on a random axis: the hit point nearest a safe-box face
                const Triangle &tr = rand_tri();
                const Vec3D p[3] = {tr.p1, tr.p2, tr.p3};
                const int a = (int)(k >> 3) % 3, hi_side = (int)(k >> 6) & 1;
                int best = 0;
                for (int v = 1; v < 3; ++v) {
                    const float c = (&p[v].x)[a], b = (&p[best].x)[a];
                    if (hi_side ? c > b : c < b) best = v;
                }
                const Vec3D cen = (1.0f / 3.0f) * (p[0] + p[1] + p[2]);
                const float w = ldexpf(U(rng), -(int)(4 + (k >> 7) % 20));
                const Vec3D target = p[best] + w * (cen - p[best]);
                o = on_tri(rand_tri());
                d = rt_normalize(target - o);
            } else if (mode >= 4 && !glass.empty()) {
                const size_t gi = (size_t)(U(rng) * glass.size()) % glass.size();
                const Triangle &tr = scene.tris[(size_t)glass[gi]];
                o = on_tri(tr);
                const long long span = mode == 4 ? (long long)glass.size() : 64;
                const long long gj = (long long)gi + (long long)((U(rng) - 0.5f) * span);
                const Triangle &to = scene.tris[(size_t)glass[(size_t)((gj % (long long)glass.size() + glass.size()) % glass.size())]];
                d = rt_normalize(on_tri(to) - o);
            } else { // a bounce: from a point on a random triangle, some grazing / axis-parallel
                const Triangle &tr = rand_tri();
                o = on_tri(tr);
                d = unit();
                if (mode == 2) {
                    const Vec3D nn = rt_normalize(rt_cross(tr.p2 - tr.p1, tr.p3 - tr.p1));
                    if (nn.x == nn.x) d = rt_normalize(d - rt_dot(d, nn) * nn + 1e-4f * (U(rng) - 0.5f) * nn);
                } else if (mode == 3 && (k & 8)) {
                    const int a = (int)(k >> 4) % 3;
                    if (a == 0) d.x = 0; else if (a == 1) d.y = 0; else d.z = 0;
                    d = rt_normalize(d);
                }
            }
            ++t.rays;
            if (d.x != d.x || d.y != d.y || d.z != d.z) continue; // (a degenerate aim: no ray)
            check_ray(h, kc, o, d, t);
        }
#pragma omp critical
        total.add(t);
    }
    return report(total);
}
