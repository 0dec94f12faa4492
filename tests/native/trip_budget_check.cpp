// trip_budget_check.cpp — the whole-call finisher's parked s_min queries under the wave's work budget
// (csrc/bvh_trace.h bvh4_query_budget, restated for the host in csrc/host/trace_host.h wave_call_budget over
// Bvh4Walk), on the library's own prepared arrays.
//
// Seeded rays are put into waves of 64 lanes; a lane takes the next ray when its query ends, as a finisher lane
// takes its path's next ray, so new queries (at the root) keep joining lanes parked at nodes and at leaves.
// For every budget given:
//
//  * every query's (s_min, tk) equals the unparked sequential query's (trace_host.h bvh4_smin) bit for bit;
//  * every query ends;
//  * no query takes more wave calls than it has bodies (node steps + leaf visits) of its own — the progress
//    rule: an unfinished lane executes at least one body in every call, whatever the budget.
//
// Rays: from the camera, bounces from random triangles (some grazing, some axis-parallel), rays that start on
// the transparent objects (chords and grazing chords), and rays that start 1e-4 off a random triangle.
//
// usage: trip_budget_check scene.txt rays seed budget [budget ...]
// exit 0 = all hold.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "host/trace_host.h"

using namespace trace_host;

namespace {

struct Ray {
    Vec3D o, d;
    float exit_;
};

struct Tally {
    long long queries = 0, mism = 0, slow = 0, unfinished = 0, calls = 0, leaf_parks = 0, ties = 0, most_trips = 0;
    double wave_bodies = 0;
};

Tally run(const rt_host::PreparedHost &h, const std::vector<Ray> &rays, int budget)
{
    Tally t;
    std::vector<Bvh4Walk> lane(64);
    std::vector<long long> ray_of(64, -1);
    size_t next = 0;
    // (every call gives every unfinished lane a body: a generous bound on the calls that still proves "ends")
    const long long call_limit = 1000 + 4096ll * (long long)rays.size();
    while (true) {
        std::vector<Bvh4Walk *> q;
        for (size_t l = 0; l < lane.size(); ++l) {
            if (ray_of[l] < 0 && next < rays.size()) {
                ray_of[l] = (long long)next;
                lane[l].start(h, rays[next].o, rays[next].d, rays[next].exit_);
                ++next;
            }
            if (ray_of[l] >= 0) q.push_back(&lane[l]);
        }
        if (q.empty()) break;
        if (++t.calls > call_limit) {
            t.unfinished = (long long)q.size() + (long long)(rays.size() - next);
            break;
        }
        const WaveTrip w = wave_call_budget(q, budget);
        t.wave_bodies += (double)(w.node_bodies + w.leaf_bodies);
        for (size_t l = 0; l < lane.size(); ++l) {
            if (ray_of[l] < 0) continue;
            Bvh4Walk &k = lane[l];
            if (k.trips > k.bodies) ++t.slow; // a call without a body of its own
            if (!k.done()) {
                t.leaf_parks += k.at_leaf();
                continue;
            }
            const Ray &r = rays[(size_t)ray_of[l]];
            const Smin ref = bvh4_smin(h, r.o, r.d, r.exit_);
            ++t.queries;
            t.ties += ref.tk == TK_TIE;
            t.most_trips = k.trips > t.most_trips ? k.trips : t.most_trips;
            if (fbits(ref.best) != fbits(k.best) || ref.tk != k.tk) {
                if (++t.mism <= 3)
                    fprintf(stderr, "MISMATCH budget %d o (%a %a %a) d (%a %a %a): sequential %a tk %d, parked %a tk %d\n",
                            budget, r.o.x, r.o.y, r.o.z, r.d.x, r.d.y, r.d.z, ref.best, ref.tk, k.best, k.tk);
            }
            ray_of[l] = -1;
        }
    }
    return t;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 5) {
        fprintf(stderr, "usage: %s scene.txt rays seed budget [budget ...]\n", argv[0]);
        return 2;
    }
    RtHostScene scene;
    Camera cam;
    rt_host::PreparedHost h;
    if (!load_prepared(argv[1], scene, cam, h) || h.bvh_depth < 0) {
        fprintf(stderr, "prepare failed / no BVH built\n");
        return 2;
    }
    const int n = (int)scene.tris.size();
    const long long want = atoll(argv[2]);
    std::vector<int> glass;
    for (int i = 0; i < n; ++i)
        if (scene.tris[(size_t)i].material.transparent) glass.push_back(i);
    std::mt19937_64 rng(strtoull(argv[3], nullptr, 10));
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    auto u = [&]() { return U(rng); };
    std::vector<Ray> rays;
    long long on_glass = 0, off_wall = 0;
    for (long long k = 0; (long long)rays.size() < want && k < 64 * want; ++k) {
        Vec3D o, d;
        const int mode = (int)(k % 8);
        if (mode == 0) { // from the camera
            o = cam.position;
            d = unit_vector(u);
        } else if (mode >= 6 && !glass.empty()) { // starts on a transparent object: a chord / a grazing chord
            const Triangle &tr = glass_chord(scene, glass, mode == 6 ? (long long)glass.size() : 64, u, o, d);
            if (mode == 7) d = grazing_chord(d, tr, u);
        } else if (mode >= 4) { // starts 1e-4 off a triangle, on either side, some nearly along it
            const Triangle &tr = scene.tris[(size_t)(u() * n) % n];
            const Vec3D nn = tri_normal(tr);
            if (nn.x != nn.x) continue;
            o = point_on(tr, u) + (u() < 0.5f ? 1e-4f : -1e-4f) * nn;
            d = unit_vector(u);
            if (mode == 5) d = grazing(d, tr, u);
        } else { // a bounce: from a point on a random triangle, some grazing / axis-parallel
            const Triangle &tr = scene.tris[(size_t)(u() * n) % n];
            o = point_on(tr, u);
            d = unit_vector(u);
            if (mode == 2) d = grazing(d, tr, u);
            else if (mode == 3 && (k & 8)) d = axis_parallel(d, (int)(k >> 4) % 3);
        }
        if (!(o.x - o.x == 0.0f && o.y - o.y == 0.0f && o.z - o.z == 0.0f && d.x - d.x == 0.0f && d.y - d.y == 0.0f &&
              d.z - d.z == 0.0f))
            continue;
        float t1, t2;
        if (!scene_box(h, o, d, t1, t2)) continue; // (no query: a miss)
        rays.push_back(Ray{o, d, t2});
        on_glass += mode >= 6 && !glass.empty();
        off_wall += mode == 4 || mode == 5;
    }
    printf("tris %d rays %zu on glass %lld off a triangle %lld\n", n, rays.size(), on_glass, off_wall);
    int bad = 0;
    for (int a = 4; a < argc; ++a) {
        const int budget = atoi(argv[a]);
        const Tally t = run(h, rays, budget);
        printf("budget %d queries %lld mismatches %lld slow %lld unfinished %lld calls %lld most calls of a query %lld "
               "parks at a leaf %lld ties %lld wave bodies per call %.2f\n",
               budget, t.queries, t.mism, t.slow, t.unfinished, t.calls, t.most_trips, t.leaf_parks, t.ties,
               t.calls ? t.wave_bodies / (double)t.calls : 0.0);
        if (t.mism || t.slow || t.unfinished || t.queries != (long long)rays.size()) bad = 1;
    }
    return bad;
}
