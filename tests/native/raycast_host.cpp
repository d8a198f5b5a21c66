// The ray-cast kernels (csrc/shm_raycast.hip.h) compiled for the host behind a thin shim: one "lane", one "wave" per brick, the launches replaced by loops.
// tests/test_raycast.py builds this with -fsanitize=address,undefined and runs the tests' rays (the degenerate ones included) through it before any GPU does:
// every index the traversal forms is checked against its allocation, whatever the floats hold.  The test includes a copy of the header without its
// #include of shm_kernels.hip.h as "shm_raycast_host.h".
// usage: raycast_host n nslabs phi.f64 rays.f64 Q grid.f64(bbox_min[3], cell) iso t_min t_max out.f64(t[Q], grad[3Q])
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define __restrict__
struct Dim3 { unsigned x, y, z; };
static Dim3 blockIdx{0, 0, 0}, threadIdx{0, 0, 0}, gridDim{1, 1, 1};
namespace shm {
constexpr int kWave = 1, kBlock = 1;
using std::max;
using std::min;
inline double block_sum(double v, double*) { return v; }
template <typename T> T __shfl_xor(T v, int, int) { return v; }
inline void atomicAdd(unsigned long long* p, unsigned long long v) { *p += v; }
}  // namespace shm
#include "shm_raycast_host.h"
using namespace shm;

template <typename T> static bool read_all(const char* path, std::vector<T>& v) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const size_t got = fread(v.data(), sizeof(T), v.size(), f);
    fclose(f);
    return got == v.size();
}

int main(int argc, char** argv) {
    if (argc != 11) return 2;
    const int n = atoi(argv[1]), ns = atoi(argv[2]);
    const int64_t Q = atoll(argv[5]);
    std::vector<double> phi((size_t)n * n * n), rays((size_t)6 * Q), grid(4);
    if (!read_all(argv[3], phi) || !read_all(argv[4], rays) || !read_all(argv[6], grid)) return 3;
    const size_t plane = (size_t)n * n;
    // the slabs in ghost layout: the high ghost plane holds the next slab's first plane, every other ghost value is NaN
    std::vector<std::vector<double>> arr((size_t)ns);
    std::vector<RaySlab<double>> tab((size_t)ns);
    for (int s = 0; s < ns; s++) {
        const int q = n / ns, r = n % ns, k0 = s * q + std::min(s, r), k1 = k0 + q + (s < r ? 1 : 0);
        arr[s].assign(plane * (size_t)(k1 - k0 + 2), NAN);
        for (int k = k0; k < std::min(k1 + 1, n); k++) std::copy(phi.begin() + k * plane, phi.begin() + (k + 1) * plane, arr[s].begin() + (k - k0 + 1) * plane);
        tab[s] = RaySlab<double>{arr[s].data(), k0, k1};
    }
    RayParams P;
    P.n = n;
    P.nb = (n - 1 + kRayBrick - 1) / kRayBrick;
    P.nslabs = ns;
    P.cell = grid[3];
    for (int a = 0; a < 3; a++) {
        P.bbox_min[a] = grid[a];
        P.hi[a] = (n - 1) * P.cell + grid[a];
    }
    P.iso = atof(argv[7]);
    P.t_min = atof(argv[8]);
    P.t_max = atof(argv[9]);
    const size_t nbricks = (size_t)P.nb * P.nb * P.nb;
    std::vector<double> minmax(2 * nbricks);
    for (size_t b = 0; b < nbricks; b++) {
        blockIdx.x = (unsigned)b;
        ray_bricks_kernel<double>(P, tab.data(), minmax.data());
    }
    blockIdx.x = 0;
    std::vector<double> o((size_t)3 * Q), d((size_t)3 * Q), out((size_t)4 * Q);
    for (int64_t q = 0; q < Q; q++)
        for (int a = 0; a < 3; a++) {
            o[3 * q + a] = rays[6 * q + a];
            d[3 * q + a] = rays[6 * q + 3 + a];
        }
    unsigned long long hits[4] = {0, 0, 0, 0};
    raycast_kernel<double, double, true>(P, Q, o.data(), d.data(), tab.data(), minmax.data(), out.data(), out.data() + Q, hits);
    FILE* f = fopen(argv[10], "wb");
    if (!f || fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 4;
    fclose(f);
    printf("hits %llu\n", hits[0]);
    return 0;
}
