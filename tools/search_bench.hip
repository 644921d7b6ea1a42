// search_bench.hip -- measurement tool (not product): times the search C-ABI
// on ONE device against the kernels it is judged by, in one process.
//   * extrema, 2^28 random u32: drhip_min_element, drhip_max_element and
//     drhip_minmax_element against drhip_reduce with DRHIP_MIN over the same
//     array (bar: min_element <= 1.15 x the reduce; minmax_element recorded);
//   * search without a match: drhip_find_if (x == a value that is absent)
//     against drhip_count_if of the same array, drhip_is_sorted_until on a
//     sorted array against drhip_count_if of that array (bar: <= 1.15 x);
//   * search with a match: drhip_find_if with the only hit at element 0, at
//     n / 1000, at n / 2 and at n - 1, as a fraction of the no-match time
//     (condition: hit at 0 < hit at n / 2 < no match).
// Three runs; in each, 3 warm-up rounds, then `reps` (default 20) timed rounds;
// every round runs every variant once (the variants alternate), HIP events on
// the segment's stream around one call; the median of a run is reported, in
// microseconds.  Every index is checked against a plain atomic reference.
// Then, without a bar: shp::min_element and shp::find_if (no match) of 2^28
// u32 on 1 and on 8 segments, end to end (host clock around the blocking call).
// Build: make -C tools search_bench.   Run: tools/search_bench [reps] [log2n]
#include <dr/shp.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#define CK(x)                                                                   \
  do {                                                                          \
    hipError_t e_ = (x);                                                        \
    if (e_ != hipSuccess) {                                                     \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      exit(1);                                                                  \
    }                                                                           \
  } while (0)
#define CD(x)                                                                      \
  do {                                                                             \
    int r_ = (x);                                                                  \
    if (r_) {                                                                      \
      fprintf(stderr, "%s:%d drhip %d %s\n", __FILE__, __LINE__, r_, drhip_last_error()); \
      exit(1);                                                                     \
    }                                                                              \
  } while (0)

__device__ inline uint64_t mix(uint64_t i, uint64_t seed) {
  uint64_t h = (i + 1) * 0x9E3779B97F4A7C15ull ^ seed;
  h ^= h >> 31;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 29;
  return h;
}
// random values below 2^31, so 0xFFFFFFFF is absent
__global__ void gen_u32(uint32_t *x, size_t n, uint64_t seed) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    x[i] = (uint32_t)(mix(i, seed) >> 33);
}
__global__ void gen_iota(uint32_t *x, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    x[i] = (uint32_t)i;
}
// res[0] = {min value, its first index}, res[1] = {max value, ~ its first index}, res[2] = {max value, its last index}
__global__ void ref_extrema(const uint32_t *x, size_t n, unsigned long long *res) {
  unsigned long long lo = ~0ull, hi1 = 0, hi2 = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long v = (unsigned long long)x[i] << 32;
    lo = min(lo, v | (uint32_t)i);
    hi1 = max(hi1, v | (uint32_t)~i);
    hi2 = max(hi2, v | (uint32_t)i);
  }
  atomicMin(res, lo);
  atomicMax(res + 1, hi1);
  atomicMax(res + 2, hi2);
}

constexpr int kWarm = 3, kRuns = 3;
constexpr uint32_t kAbsent = 0xFFFFFFFFu;

struct Variant {
  std::string name;
  std::function<void()> before, call, after; // before / after run outside the timed region
  unsigned long long want0 = 0, want1 = 0;
  int words = 1; // index words to check (0: none)
  std::vector<float> t;
  double med[kRuns] = {};
};

int main(int argc, char **argv) {
  const int reps = argc > 1 ? std::max(1, atoi(argv[1])) : 20;
  const int log2n = argc > 2 ? atoi(argv[2]) : 28;
  const size_t n = size_t(1) << log2n;
  shp::init(std::vector<int>{0});
  hipStream_t st = shp::stream(0);
  printf("search_bench: n = 2^%d u32, %d runs of %d warm-up + %d timed rounds, every variant once per round, "
         "median per run in us, HIP events\n", log2n, kRuns, kWarm, reps);

  uint32_t *x, *sorted;
  CK(hipMalloc(&x, n * 4));
  CK(hipMalloc(&sorted, n * 4));
  hipLaunchKernelGGL(gen_u32, dim3(4096), dim3(256), 0, st, x, n, 12345ull);
  hipLaunchKernelGGL(gen_iota, dim3(4096), dim3(256), 0, st, sorted, n);
  unsigned long long *idx, *d_ref, ref[3];
  uint32_t *red, *hit_val, *keep;
  CK(hipHostMalloc(&idx, 16));
  CK(hipHostMalloc(&hit_val, 4));
  CK(hipHostMalloc(&keep, 4));
  *hit_val = kAbsent;
  CK(hipMalloc(&d_ref, 24));
  CK(hipMalloc(&red, 8));
  const unsigned long long init[3] = {~0ull, 0, 0};
  CK(hipMemcpyAsync(d_ref, init, 24, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(ref_extrema, dim3(2048), dim3(256), 0, st, x, n, d_ref);
  CK(hipMemcpyAsync(ref, d_ref, 24, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  const unsigned long long first_min = (uint32_t)ref[0], first_max = (uint32_t)~ref[1], last_max = (uint32_t)ref[2];

  std::vector<Variant> vs;
  auto add = [&](const char *name, std::function<void()> call, int words, unsigned long long w0, unsigned long long w1) {
    Variant v;
    v.name = name, v.call = call, v.words = words, v.want0 = w0, v.want1 = w1;
    vs.push_back(v);
  };
  uint64_t *index = (uint64_t *)idx;
  add("drhip_reduce u32 min            ", [=] { CD(drhip_reduce(0, DRHIP_U32, DRHIP_MIN, x, n, red)); }, 0, 0, 0);
  add("drhip_min_element               ", [=] { CD(drhip_min_element(0, DRHIP_U32, x, n, index)); }, 1, first_min, 0);
  add("drhip_max_element               ", [=] { CD(drhip_max_element(0, DRHIP_U32, x, n, index)); }, 1, first_max, 0);
  add("drhip_minmax_element            ", [=] { CD(drhip_minmax_element(0, DRHIP_U32, x, n, index)); }, 2, first_min, last_max);
  add("drhip_count_if eq absent        ", [=] { CD(drhip_count_if(0, DRHIP_U32, DRHIP_EQ, x, n, &kAbsent, index)); }, 1, 0, 0);
  add("drhip_find_if no match          ", [=] { CD(drhip_find_if(0, DRHIP_U32, DRHIP_EQ, x, n, &kAbsent, index)); }, 1, n, 0);
  const size_t hits[4] = {0, n / 1000, n / 2, n - 1};
  const char *hit_names[4] = {"drhip_find_if hit at 0          ", "drhip_find_if hit at n/1000     ",
                              "drhip_find_if hit at n/2        ", "drhip_find_if hit at n-1        "};
  for (int h = 0; h < 4; h++) {
    add(hit_names[h], [=] { CD(drhip_find_if(0, DRHIP_U32, DRHIP_EQ, x, n, &kAbsent, index)); }, 1, hits[h], 0);
    const size_t p = hits[h];
    vs.back().before = [=] {
      CK(hipMemcpyAsync(keep, x + p, 4, hipMemcpyDeviceToHost, st));
      CK(hipMemcpyAsync(x + p, hit_val, 4, hipMemcpyHostToDevice, st));
      CK(hipStreamSynchronize(st));
    };
    vs.back().after = [=] { CK(hipMemcpyAsync(x + p, keep, 4, hipMemcpyHostToDevice, st)); CK(hipStreamSynchronize(st)); };
  }
  add("drhip_count_if eq absent, sorted", [=] { CD(drhip_count_if(0, DRHIP_U32, DRHIP_EQ, sorted, n, &kAbsent, index)); }, 1, 0, 0);
  add("drhip_is_sorted_until, sorted   ", [=] { CD(drhip_is_sorted_until(0, DRHIP_U32, sorted, n, index)); }, 1, n, 0);

  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  int bad = 0;
  for (int run = 0; run < kRuns; run++) {
    for (auto &v : vs) v.t.clear();
    for (int r = -kWarm; r < reps; r++)
      for (auto &v : vs) {
        if (v.before) v.before();
        idx[0] = idx[1] = 0xDEADull;
        CK(hipEventRecord(e0, st));
        v.call();
        CK(hipEventRecord(e1, st));
        CK(hipStreamSynchronize(st));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 0) v.t.push_back(ms * 1000.f);
        if (v.after) v.after();
        const bool ok = v.words == 0 || (idx[0] == v.want0 && (v.words == 1 || idx[1] == v.want1));
        if (!ok && r == reps - 1) {
          printf("WRONG: %s gave %llu %llu, want %llu %llu\n", v.name.c_str(), idx[0], idx[1], v.want0, v.want1);
          bad++;
        }
      }
    for (auto &v : vs) {
      std::sort(v.t.begin(), v.t.end());
      v.med[run] = v.t[v.t.size() / 2];
    }
  }
  for (auto &v : vs) printf("%s %9.1f %9.1f %9.1f us\n", v.name.c_str(), v.med[0], v.med[1], v.med[2]);
  auto med = [&](const char *prefix, int run) {
    for (auto &v : vs)
      if (v.name.rfind(prefix, 0) == 0) return v.med[run];
    return 0.0;
  };
  for (int run = 0; run < kRuns; run++) {
    const double red_t = med("drhip_reduce", run), cnt = med("drhip_count_if eq absent  ", run),
                 cnts = med("drhip_count_if eq absent, sorted", run), none = med("drhip_find_if no match", run);
    printf("run %d: min_element / reduce %.3f (bar 1.15: %s), max_element / reduce %.3f, minmax_element / reduce %.3f\n", run,
           med("drhip_min_element", run) / red_t, med("drhip_min_element", run) <= 1.15 * red_t ? "met" : "MISSED",
           med("drhip_max_element", run) / red_t, med("drhip_minmax_element", run) / red_t);
    printf("run %d: find_if no match / count_if %.3f (bar 1.15: %s), is_sorted_until / count_if %.3f (bar 1.15: %s)\n", run,
           none / cnt, none <= 1.15 * cnt ? "met" : "MISSED", med("drhip_is_sorted_until", run) / cnts,
           med("drhip_is_sorted_until", run) <= 1.15 * cnts ? "met" : "MISSED");
    const double h0 = med("drhip_find_if hit at 0", run), h1 = med("drhip_find_if hit at n/1000", run),
                 h2 = med("drhip_find_if hit at n/2", run), h3 = med("drhip_find_if hit at n-1", run);
    printf("run %d: find_if hit at 0, n/1000, n/2, n-1 as a fraction of no match: %.4f %.4f %.4f %.4f; "
           "hit at 0 < hit at n/2 < no match: %s\n", run, h0 / none, h1 / none, h2 / none, h3 / none,
           h0 < h2 && h2 < none ? "holds" : "FAILS");
  }
  fflush(stdout);
  CK(hipFree(x));
  CK(hipFree(sorted));
  CK(hipFree(d_ref));
  CK(hipFree(red));
  CK(hipHostFree(idx));
  CK(hipHostFree(hit_val));
  CK(hipHostFree(keep));
  shp::finalize();

  // the header layer end to end, 1 and 8 segments (duplicated on the visible devices)
  const size_t ndev = shp::get_numa_devices().size();
  for (std::size_t segs : {std::size_t(1), std::size_t(8)}) {
    shp::init(shp::get_duplicated_devices(shp::get_numa_devices(), segs));
    {
      shp::distributed_vector<uint32_t> in(n);
      for (auto &s : in.segments())
        hipLaunchKernelGGL(gen_u32, dim3(4096), dim3(256), 0, shp::stream(s.rank()), s.data(), s.size(), 777ull + s.rank());
      shp::sync_all();
      auto absent = [] __device__(uint32_t v) { return v == 0xFFFFFFFFu; };
      std::vector<double> tm, tf;
      std::size_t got_min = 0, got_find = 0;
      const int r2 = std::min(reps, 10);
      for (int r = -kWarm; r < r2; r++) {
        auto t0 = std::chrono::steady_clock::now();
        auto it = shp::min_element(shp::par_unseq, in);
        auto t1 = std::chrono::steady_clock::now();
        auto jt = shp::find_if(shp::par_unseq, in, absent);
        auto t2 = std::chrono::steady_clock::now();
        got_min = (std::size_t)(it - in.begin());
        got_find = (std::size_t)(jt - in.begin());
        if (r >= 0) {
          tm.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
          tf.push_back(std::chrono::duration<double, std::micro>(t2 - t1).count());
        }
      }
      std::sort(tm.begin(), tm.end());
      std::sort(tf.begin(), tf.end());
      // the minimum's value must be the reduce's, and nothing before it may equal it
      const uint32_t lo = shp::reduce(shp::par_unseq, in, 0xFFFFFFFFu, shp::minimum<uint32_t>{});
      auto is_lo = [lo] __device__(uint32_t v) { return v == lo; };
      const std::size_t first_lo = (std::size_t)(shp::find_if(shp::par_unseq, in, is_lo) - in.begin());
      const bool ok = got_min == first_lo && got_find == n;
      printf("shp::min_element n=2^%d, %zu segment%s on %zu device%s, end to end: %9.1f us (%.1f-%.1f)  index=%zu%s\n", log2n,
             segs, segs > 1 ? "s" : "", std::min(segs, ndev), segs > 1 && ndev > 1 ? "s" : "", tm[tm.size() / 2], tm.front(),
             tm.back(), got_min, ok ? "  ok" : "  WRONG");
      printf("shp::find_if no match n=2^%d, %zu segment%s on %zu device%s, end to end: %9.1f us (%.1f-%.1f)\n", log2n, segs,
             segs > 1 ? "s" : "", std::min(segs, ndev), segs > 1 && ndev > 1 ? "s" : "", tf[tf.size() / 2], tf.front(),
             tf.back());
      bad += !ok;
    }
    shp::finalize();
  }
  if (ndev < 2) printf("segments on distinct GPUs: unmeasured (one GPU visible)\n");
  return bad ? 1 : 0;
}
