// kd_cert_check.cpp — the T* certificate (csrc/bvh_common.h rt_kd_cert) checked on the
// library's own prepared arrays, ray by ray, against the plain KD traversal:
//
//  * tables: every safe box has the final-pass property (every KD leaf whose closed cell meets it lists
//    the slot's triangle — an independent recursive sweep, not scene_prepare's), every split value is a
//    member of its axis' hash set, the load factor is <= 0.5 (shipped: <= 0.25), and -0 finds +0;
//  * rays: the bounded traversal as the kernels run it (restated in csrc/host/trace_host.h) — the s_min query,
//    then the certificate, then (uncertified) the bounded KD descent, IEEE divisions, a T* entry that does
//    not pass ending the program — returns the plain KD traversal's triangle and barycentrics
//    bit for bit; a certified ray's descent is run too and must agree;
//  * slack: for every ray whose hit point passes the box test, the shipped delta (rt_cert_delta) is at
//    least 4x the derived bound e_P + delta_desc + the box comparison's own rounding, evaluated from
//    the ray's actual magnitudes in double.
//
// Ray sets: the mix of wide_smin_check.cpp, from trace_host.h's ray makers (camera rays, bounces off random
// triangles — some grazing, some axis-parallel —, chords of transparent objects), rays whose origin coordinate IS a split value
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

#include "host/trace_host.h"

using namespace trace_host;

namespace {

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
    const Hit plain = kd_plain(h, o, d, t1, t2);
    if (plain.tri >= 0) ++t.hits;
    const Smin q = bvh4_smin(h, o, d, t2);
    const float s_min = q.best;
    const int tk = q.tk;
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
        const Hit desc = kd_descent<IEEE_DIV, HARD_FAILURE>(h, o, d, t1, t2, s_min, tstar_of(h, tk));
        if (why == RT_CERT_OK) {
            ++t.certified;
            const RtIsectBary &R = h.bvh_bary[tk];
            if (rt_tri_bary(R.b, R.c, R.d, bitsf(R.rd), o, d, s_min, got.b[0], got.b[1], got.b[2])) got.tri = (int)R.tri;
            if (!same_hit(got, desc)) ++t.cert_descent_mism;
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
    if (!same_hit(got, plain)) {
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
    std::vector<float> v;
    if (!read_rays_f32(path, v)) return 2;
    const long long n = (long long)(v.size() / 6);
    const RtKdCert kc = h.kd_cert();
    Tally total;
#pragma omp parallel
    {
        Tally t;
#pragma omp for schedule(dynamic, 1024)
        for (long long k = 0; k < n; ++k) {
            ++t.rays;
            check_ray(h, kc, ray_o(v, (size_t)k), ray_d(v, (size_t)k), t);
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
    rt_host::PreparedHost h;
    double t_prep = 0;
    if (!load_prepared(argv[1], scene, cam, h, &t_prep) || h.bvh_depth < 0 || h.kd_safe.empty()) {
        fprintf(stderr, "prepare failed / no BVH or certificate tables built\n");
        return 2;
    }
    const int n = (int)scene.tris.size();
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
        auto u = [&]() { return U(rng); };
        auto unit = [&]() { return unit_vector(u); };
        auto on_tri = [&](const Triangle &tr) { return point_on(tr, u); };
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
                (void)glass_chord(scene, glass, mode == 4 ? (long long)glass.size() : 64, u, o, d);
            } else { // a bounce: from a point on a random triangle, some grazing / axis-parallel
                const Triangle &tr = rand_tri();
                o = on_tri(tr);
                d = unit();
                if (mode == 2) d = grazing(d, tr, u);
                else if (mode == 3 && (k & 8)) d = axis_parallel(d, (int)(k >> 4) % 3);
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
