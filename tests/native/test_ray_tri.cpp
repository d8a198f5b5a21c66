// Host test of csrc/shm_ray_tri.h, the ray / triangle rule of shm_grid_mesh_raycast: the kernel calls the same functions.  No GPU; built by
// tests/test_mesh_raycast.py with g++, once plain and once under AddressSanitizer + UBSan, and run stand-alone.
//
//   1. a ray through an interior point: hit, with the t and the barycentrics of the point
//   2. a ray through a point of an edge shared by two triangles that face the same way: exactly one of them, for every axis, sense and winding
//   3. a ray through a vertex shared by a closed fan (the apex of an octahedron, the corner of a cube): one triangle from inside, two crossings from outside
//   4. a ray through a silhouette edge (two triangles that face opposite ways along the ray): 0 or 2
//   5. zero-area triangles (a point, a segment, collinear corners), hit head-on and from within their line: never
//   6. det has the sign of -(d . N) on random hits
//   7. rt_edge(Q, P) == -rt_edge(P, Q) bit for bit, and the adjusted signs are opposite, on 10^5 random pairs of sheared corners (half of them with
//      coordinates from a small integer set, where zeros and ties abound)
//   8. closed meshes (octahedron, cube of 12 triangles) under rays from lattice points through lattice points -- vertices, edges and faces are hit exactly
//      all the time, and the rays kept are those whose shear is exact: the count is odd from inside and even from outside, bar none
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../signed-heat-3d_amd/csrc/shm_ray_tri.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}
double uniform(double lo, double hi) { return lo + (hi - lo) * (double)(rnd() >> 11) * 0x1p-53; }

int failures = 0;
void fail(const char* what, double a, double b) {
    if (failures < 20) std::printf("FAIL %s: %.17g against %.17g\n", what, a, b);
    failures++;
}

struct V3 {
    double x[3];
};
struct Tri {
    V3 a, b, c;
};

struct Hit {
    bool hit;
    double t, u, v, det;
};
Hit cast(const V3& o, const V3& d, const Tri& T, double t_min = 0., double t_max = INFINITY) {
    const shm::RtRay R = shm::rt_setup(d.x);
    double A[3], B[3], C[3];
    for (int a = 0; a < 3; a++) {
        A[a] = T.a.x[a] - o.x[a];
        B[a] = T.b.x[a] - o.x[a];
        C[a] = T.c.x[a] - o.x[a];
    }
    Hit h{false, 0., 0., 0., 0.};
    h.hit = shm::rt_hit(R, A, B, C, t_min, t_max, &h.t, &h.u, &h.v, &h.det);
    return h;
}
int count(const V3& o, const V3& d, const std::vector<Tri>& M, double t_min = 0., double t_max = INFINITY) {
    int c = 0;
    for (const Tri& T : M) c += cast(o, d, T, t_min, t_max).hit ? 1 : 0;
    return c;
}

std::vector<Tri> octahedron() {
    const V3 px{{1, 0, 0}}, nx{{-1, 0, 0}}, py{{0, 1, 0}}, ny{{0, -1, 0}}, pz{{0, 0, 1}}, nz{{0, 0, -1}};
    return {{px, py, pz}, {py, nx, pz}, {nx, ny, pz}, {ny, px, pz}, {py, px, nz}, {nx, py, nz}, {ny, nx, nz}, {px, ny, nz}};
}
std::vector<Tri> cube() {   // [-1, 1]^3, outward
    std::vector<Tri> M;
    for (int a = 0; a < 3; a++)
        for (int s = -1; s <= 1; s += 2) {
            const int b = (a + 1) % 3, c = (a + 2) % 3;
            V3 p[4];
            const int cb[4] = {-1, 1, 1, -1}, cc[4] = {-1, -1, 1, 1};
            for (int i = 0; i < 4; i++) {
                p[i].x[a] = s;
                p[i].x[b] = cb[i];
                p[i].x[c] = cc[i];
            }
            if (s > 0) {
                M.push_back({p[0], p[1], p[2]});
                M.push_back({p[0], p[2], p[3]});
            } else {
                M.push_back({p[0], p[2], p[1]});
                M.push_back({p[0], p[3], p[2]});
            }
        }
    return M;
}

void interior() {
    const Tri T{{{0, 0, 2}}, {{4, 0, 2}}, {{0, 4, 2}}};
    const Hit h = cast({{1, 1, 0}}, {{0, 0, 0.5}}, T);
    if (!h.hit) return fail("interior: no hit", 0, 1);
    if (h.t != 4.) fail("interior t", h.t, 4.);
    if (h.u != 0.25 || h.v != 0.25) fail("interior (u, v)", h.u, h.v);
    if (cast({{1, 1, 0}}, {{0, 0, 0.5}}, T, 0., 3.9).hit) fail("interior: hit beyond t_max", 0, 0);
    if (cast({{1, 1, 0}}, {{0, 0, 0.5}}, T, 4.1, INFINITY).hit) fail("interior: hit before t_min", 0, 0);
    if (!cast({{1, 1, 0}}, {{0, 0, 0.5}}, T, 4., 4.).hit) fail("interior: t_min = t = t_max is a hit", 0, 0);
    if (cast({{1, 1, 0}}, {{0, 0, -0.5}}, T).hit) fail("interior: hit behind the origin", 0, 0);
    if (!cast({{1, 1, 4}}, {{0, 0, -1}}, T).hit) fail("interior: the back face is hit as well", 0, 0);
    if (cast({{3, 3, 0}}, {{0, 0, 1}}, T).hit) fail("interior: a ray beside the triangle", 0, 0);
}

// two triangles of one plane perpendicular to `axis`, sharing the diagonal; rays through points of the diagonal, its end points included
void shared_edge() {
    for (int axis = 0; axis < 3; axis++)
        for (int sense = -1; sense <= 1; sense += 2)
            for (int wind = 0; wind < 2; wind++)
                for (int tilt = 0; tilt < 3; tilt++) {
                    const int b = (axis + 1) % 3, c = (axis + 2) % 3;
                    V3 p[4];
                    const double cb[4] = {0, 4, 4, 0}, cc[4] = {0, 0, 4, 4};
                    for (int i = 0; i < 4; i++) {
                        p[i].x[axis] = 3;
                        p[i].x[b] = cb[i];
                        p[i].x[c] = cc[i];
                    }
                    std::vector<Tri> M = wind ? std::vector<Tri>{{p[0], p[1], p[2]}, {p[0], p[2], p[3]}} : std::vector<Tri>{{p[0], p[2], p[1]}, {p[0], p[3], p[2]}};
                    for (double s = 1.; s <= 3.; s += 0.5) {   // interior points of the diagonal p0 p2
                        V3 target{}, o{}, d{};
                        target.x[axis] = 3;
                        target.x[b] = s;
                        target.x[c] = s;
                        o = target;
                        o.x[axis] = 3 - 2 * sense;
                        if (tilt) {   // an oblique ray through the same point: offsets that are exact
                            o.x[b] -= tilt == 1 ? 1 : -0.5;
                            o.x[c] -= tilt == 1 ? 0.5 : 1;
                        }
                        for (int a = 0; a < 3; a++) d.x[a] = target.x[a] - o.x[a];
                        const int n = count(o, d, M);
                        if (n != 1) fail("shared edge: count", n, 1);
                    }
                }
}

void shared_vertex() {
    const std::vector<Tri> O = octahedron(), Cu = cube();
    const V3 dirs[6] = {{{1, 0, 0}}, {{-1, 0, 0}}, {{0, 1, 0}}, {{0, -1, 0}}, {{0, 0, 1}}, {{0, 0, -1}}};
    for (const V3& d : dirs) {
        int n = count({{0, 0, 0}}, d, O);
        if (n != 1) fail("octahedron apex from inside", n, 1);
        V3 o{{-3 * d.x[0], -3 * d.x[1], -3 * d.x[2]}};
        n = count(o, d, O);
        if (n != 2) fail("octahedron apexes from outside", n, 2);
        V3 off{{0.25, 0.25, 0.25}};   // from an interior point that is not the centre, towards an apex
        V3 dd{{d.x[0] - off.x[0], d.x[1] - off.x[1], d.x[2] - off.x[2]}};
        n = count(off, dd, O);
        if (n != 1) fail("octahedron apex from an interior point", n, 1);
    }
    for (int sx = -1; sx <= 1; sx += 2)
        for (int sy = -1; sy <= 1; sy += 2)
            for (int sz = -1; sz <= 1; sz += 2) {
                const V3 d{{(double)sx, (double)sy, (double)sz}};
                int n = count({{0, 0, 0}}, d, Cu);
                if (n != 1) fail("cube corner from inside", n, 1);
                n = count({{-2. * sx, -2. * sy, -2. * sz}}, d, Cu);
                if (n != 2) fail("cube corners from outside", n, 2);
            }
}

// a roof: two triangles that meet in the ridge y = 0, z = 1 and fall away to both sides; a ray along +y at the ridge's height grazes it
void silhouette() {
    for (int flip = 0; flip < 2; flip++) {
        const V3 r0{{0, 0, 1}}, r1{{4, 0, 1}}, l{{2, -2, 0}}, r{{2, 2, 0}};
        std::vector<Tri> M = flip ? std::vector<Tri>{{r0, r1, l}, {r1, r0, r}} : std::vector<Tri>{{r1, r0, l}, {r0, r1, r}};
        for (double x = 0.5; x < 4.; x += 0.5)
            for (int sense = -1; sense <= 1; sense += 2) {
                const int n = count({{x, -3. * sense, 1}}, {{0, (double)sense, 0}}, M);
                if (n != 0 && n != 2) fail("silhouette edge: count", n, 0);
                const int nz = count({{x, 0, 3. * sense + 1}}, {{0, 0, -(double)sense}}, M);   // from above / below through the ridge: a crossing
                if (nz != 1) fail("ridge seen from above: count", nz, 1);
            }
    }
}

void zero_area() {
    const V3 p{{1, 1, 2}}, q{{3, 1, 2}}, m{{2, 1, 2}}, far{{5, 1, 2}};
    const Tri pts[] = {{p, p, p}, {p, q, p}, {p, p, q}, {p, m, q}, {p, q, far}, {q, p, m}};
    for (const Tri& T : pts) {
        if (cast({{1, 1, 0}}, {{0, 0, 1}}, T).hit) fail("zero area: hit head-on at a corner", 0, 0);
        if (cast({{2, 1, 0}}, {{0, 0, 1}}, T).hit) fail("zero area: hit head-on inside the segment", 0, 0);
        if (cast({{-1, 1, 2}}, {{1, 0, 0}}, T).hit) fail("zero area: hit along its own line", 0, 0);
        if (cast({{0, 0, 0}}, {{2, 1, 2}}, T).hit) fail("zero area: hit by an oblique ray through it", 0, 0);
    }
    // a proper triangle seen from within its plane, along a grid direction: the three edge functions vanish exactly
    const Tri flat{{{0, 0, 2}}, {{4, 0, 2}}, {{0, 4, 2}}};
    if (cast({{-1, 1, 2}}, {{1, 0, 0}}, flat).hit) fail("edge-on: hit from within the plane", 0, 0);
    if (cast({{-1, -1, 2}}, {{1, 1, 0}}, flat).hit) fail("edge-on: hit from within the plane, diagonal", 0, 0);
}

void det_sign() {
    int hits = 0;
    for (int it = 0; it < 200000 && hits < 20000; it++) {
        Tri T;
        for (V3* p : {&T.a, &T.b, &T.c})
            for (int a = 0; a < 3; a++) p->x[a] = uniform(-1, 1);
        V3 o, d;
        for (int a = 0; a < 3; a++) {
            o.x[a] = uniform(-2, 2);
            d.x[a] = uniform(-1, 1);
        }
        const Hit h = cast(o, d, T, -INFINITY, INFINITY);
        if (!h.hit) continue;
        hits++;
        const double e1[3] = {T.b.x[0] - T.a.x[0], T.b.x[1] - T.a.x[1], T.b.x[2] - T.a.x[2]}, e2[3] = {T.c.x[0] - T.a.x[0], T.c.x[1] - T.a.x[1], T.c.x[2] - T.a.x[2]};
        const double N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double dn = d.x[0] * N[0] + d.x[1] * N[1] + d.x[2] * N[2];
        if (std::fabs(dn) < 1e-9) continue;
        if ((h.det < 0.) != (dn > 0.)) fail("det against -(d . N)", h.det, dn);
        // and the point: o + t d = (1 - u - v) A + u B + v C
        for (int a = 0; a < 3; a++) {
            const double lhs = o.x[a] + h.t * d.x[a], rhs = (1 - h.u - h.v) * T.a.x[a] + h.u * T.b.x[a] + h.v * T.c.x[a];
            if (std::fabs(lhs - rhs) > 1e-9 * (1 + std::fabs(h.t))) fail("hit point against the barycentrics", lhs, rhs);
        }
    }
    if (hits < 1000) fail("det_sign: too few hits", hits, 1000);
}

void negation() {
    for (int it = 0; it < 100000; it++) {
        double P[2], Q[2];
        if (it & 1) {
            V3 d, p, q;
            for (int a = 0; a < 3; a++) {
                d.x[a] = uniform(-1, 1);
                p.x[a] = uniform(-3, 3);
                q.x[a] = uniform(-3, 3);
            }
            const shm::RtRay R = shm::rt_setup(d.x);
            double z;
            shm::rt_shear(R, p.x, &P[0], &P[1], &z);
            shm::rt_shear(R, q.x, &Q[0], &Q[1], &z);
        } else {
            for (int a = 0; a < 2; a++) {
                P[a] = (double)((int)(rnd() % 5) - 2);
                Q[a] = (double)((int)(rnd() % 5) - 2);
            }
        }
        const double e = shm::rt_edge(P[0], P[1], Q[0], Q[1]), r = shm::rt_edge(Q[0], Q[1], P[0], P[1]);
        if (!(e == -r)) fail("edge function of the reversed edge", e, r);
        const int se = shm::rt_edge_sign(e, P[0], P[1], Q[0], Q[1]), sr = shm::rt_edge_sign(r, Q[0], Q[1], P[0], P[1]);
        if (se != -sr) fail("adjusted sign of the reversed edge", se, sr);
        if (se == 0 && !(P[0] == Q[0] && P[1] == Q[1])) fail("adjusted sign zero for distinct corners", P[0], Q[0]);
    }
}

void closed_parity() {
    const std::vector<Tri> O = octahedron(), Cu = cube();
    long rays = 0;
    for (int mesh = 0; mesh < 2; mesh++) {
        const std::vector<Tri>& M = mesh ? Cu : O;
        // lattice of quarter steps: origins in [-2, 2]^3, targets in [-1, 1]^3
        for (int it = 0; it < 400000; it++) {
            V3 o, g, d;
            for (int a = 0; a < 3; a++) {
                o.x[a] = 0.25 * ((int)(rnd() % 17) - 8);
                g.x[a] = 0.25 * ((int)(rnd() % 9) - 4);
                d.x[a] = g.x[a] - o.x[a];
            }
            if (d.x[0] == 0. && d.x[1] == 0. && d.x[2] == 0.) continue;
            const double l1 = std::fabs(o.x[0]) + std::fabs(o.x[1]) + std::fabs(o.x[2]), linf = std::fmax(std::fabs(o.x[0]), std::fmax(std::fabs(o.x[1]), std::fabs(o.x[2])));
            const double m = mesh ? linf : l1;
            if (m == 1.) continue;   // an origin on the surface is neither
            // rays whose shear is exact (the quotients are dyadic), so that every sheared corner and edge function is exact: under rounding a ray that
            // lies in a face's plane sees that face as a needle of width 1e-17 through itself, and noise decides (shm_mesh_ray_walk.h names the case)
            const shm::RtRay R = shm::rt_setup(d.x);
            const double dz = shm::rt_pick(d.x[0], d.x[1], d.x[2], R.kz);
            if (R.Sx * dz != shm::rt_pick(d.x[0], d.x[1], d.x[2], R.kx) || R.Sy * dz != shm::rt_pick(d.x[0], d.x[1], d.x[2], R.ky)) continue;
            if (std::fabs(R.Sx) * 64 != std::floor(std::fabs(R.Sx) * 64) || std::fabs(R.Sy) * 64 != std::floor(std::fabs(R.Sy) * 64)) continue;
            const int n = count(o, d, M);
            rays++;
            if ((n & 1) != (m < 1. ? 1 : 0)) fail(mesh ? "cube parity" : "octahedron parity", n, m);
        }
    }
    if (rays < 50000) fail("closed_parity: too few rays", (double)rays, 50000);
}

}  // namespace

int main() {
    interior();
    shared_edge();
    shared_vertex();
    silhouette();
    zero_area();
    det_sign();
    negation();
    closed_parity();
    if (failures) {
        std::printf("%d FAILURES\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
