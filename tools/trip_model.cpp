// trip_model.cpp — what a finisher wave executes per loop trip for its parked s_min queries, on the host:
// the oracle's path-traced rays (tools/dump_rays.py) in waves of 64 lanes, a lane taking the next ray when
// its query ends, replayed under two parking rules (csrc/host/trace_host.h):
//
//   lane cap C   bvh4_query<PARK>: a lane parks in front of its (C + 1)-th node step of the call; leaf visits
//                are not counted and the lanes' node runs do not line up (wave_call_lane_cap)
//   budget W     bvh4_query_budget: the wave executes one body at a time — a node step or a leaf visit,
//                whichever has more lanes waiting — and parks every unfinished query after W bodies
//                (wave_call_budget)
//
// Per rule: the bodies the wave executes per trip (node-phase iterations, leaf visits, and the visits' 4-entry
// chunks), their mean, p90, p99 and maximum, the bodies of a lane's own per trip, the trips a ray's query takes,
// the share of a trip's lanes whose query ends in it, and wave bodies per ray (the figure that costs VALU).
// Only rays that run the query are replayed (inside the scene box, rt_bounded_ray).  The model knows nothing
// of a trip's fixed cost (claims, shading, the KD descents): it picks which budgets are worth building.
// Experiment tooling, not product code.
//
// usage: trip_model scene.txt rays.f32 [cap] [first budget] [last budget]
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "host/trace_host.h"

using namespace trace_host;

namespace {

struct Ray {
    Vec3D o, d;
    float exit_;
};

struct Stats {
    std::vector<int> wave_bodies; // per trip
    long long node = 0, leaf = 0, chunks = 0, lane_bodies = 0, lane_trips = 0, finished = 0, rays = 0, ray_trips = 0,
              most_trips = 0;
};

template <class Call>
Stats replay(const rt_host::PreparedHost &h, const std::vector<Ray> &rays, Call call)
{
    Stats s;
    std::vector<Bvh4Walk> lane(64);
    std::vector<char> busy(64, 0);
    size_t next = 0;
    while (true) {
        std::vector<Bvh4Walk *> q;
        for (size_t l = 0; l < lane.size(); ++l) {
            if (!busy[l] && next < rays.size()) {
                lane[l].start(h, rays[next].o, rays[next].d, rays[next].exit_);
                busy[l] = 1;
                ++next;
            }
            if (busy[l]) q.push_back(&lane[l]);
        }
        // (the tail, where the list has run out and the wave empties, is no steady state: left out)
        if (q.size() < lane.size()) break;
        const WaveTrip w = call(q);
        s.wave_bodies.push_back((int)(w.node_bodies + w.leaf_bodies));
        s.node += w.node_bodies;
        s.leaf += w.leaf_bodies;
        s.chunks += w.leaf_chunks;
        s.lane_bodies += w.lane_bodies;
        s.lane_trips += w.lanes;
        s.finished += w.finished;
        for (size_t l = 0; l < lane.size(); ++l)
            if (lane[l].done()) {
                ++s.rays;
                s.ray_trips += lane[l].trips;
                s.most_trips = std::max(s.most_trips, lane[l].trips);
                busy[l] = 0;
            }
    }
    return s;
}

void report(const char *rule, int v, Stats &s)
{
    const double T = s.wave_bodies.empty() ? 1.0 : (double)s.wave_bodies.size(), R = s.rays ? (double)s.rays : 1.0;
    std::sort(s.wave_bodies.begin(), s.wave_bodies.end());
    auto pct = [&](double p) { return s.wave_bodies.empty() ? 0 : s.wave_bodies[(size_t)(p * (T - 1))]; };
    printf("%-8s %2d | wave bodies/trip %6.2f (node %5.2f leaf %5.2f, leaf chunks %5.2f) p90 %3d p99 %3d max %3d | "
           "lane bodies/trip %5.2f | trips/ray %5.2f (most %lld) | lanes finishing/trip %.3f | wave bodies/ray %6.3f "
           "chunk-weighted %6.3f\n",
           rule, v, (double)(s.node + s.leaf) / T, (double)s.node / T, (double)s.leaf / T, (double)s.chunks / T,
           pct(0.9), pct(0.99), pct(1.0), (double)s.lane_bodies / (double)(s.lane_trips ? s.lane_trips : 1),
           (double)s.ray_trips / R, s.most_trips, (double)s.finished / (double)(s.lane_trips ? s.lane_trips : 1),
           (double)(s.node + s.leaf) / R, (double)(s.node + s.chunks) / R);
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 3) {
        fprintf(stderr, "usage: %s scene.txt rays.f32 [cap] [first budget] [last budget]\n", argv[0]);
        return 2;
    }
    RtHostScene scene;
    Camera cam;
    rt_host::PreparedHost h;
    if (!load_prepared(argv[1], scene, cam, h) || h.bvh_depth < 0) {
        fprintf(stderr, "prepare failed / no BVH built\n");
        return 2;
    }
    std::vector<float> v;
    if (!read_rays_f32(argv[2], v)) return 2;
    const int cap = argc > 3 ? atoi(argv[3]) : 6, b0 = argc > 4 ? atoi(argv[4]) : 4, b1 = argc > 5 ? atoi(argv[5]) : 16;
    std::vector<Ray> rays;
    for (size_t i = 0; i < v.size() / 6; ++i) {
        const Vec3D o = ray_o(v, i), d = ray_d(v, i);
        float t1, t2;
        if (!scene_box(h, o, d, t1, t2) || !rt_bounded_ray(o, d, h.split_vals.data(), h.split_off)) continue;
        rays.push_back(Ray{o, d, t2});
    }
    // the unparked query's own bodies per ray (what no rule changes)
    struct Count : NoObserver {
        long long nodes = 0, leaves = 0;
        void bvh_node() { ++nodes; }
        void bvh_leaf() { ++leaves; }
    } c;
    for (const Ray &r : rays) (void)bvh4_smin(h, r.o, r.d, r.exit_, c);
    printf("tris %zu rays %zu of %zu run the query; per ray %.2f node steps %.2f leaf visits\n", scene.tris.size(),
           rays.size(), v.size() / 6, (double)c.nodes / (double)rays.size(), (double)c.leaves / (double)rays.size());
    Stats s = replay(h, rays, [&](std::vector<Bvh4Walk *> &q) { return wave_call_lane_cap(q, cap); });
    report("lane cap", cap, s);
    for (int b = b0; b <= b1; ++b) {
        Stats t = replay(h, rays, [&](std::vector<Bvh4Walk *> &q) { return wave_call_budget(q, b); });
        report("budget", b, t);
    }
    return 0;
}
