// copy_if_bench.hip -- measurement tool (not product): times the selection
// C-ABI on ONE device against the kernels it is judged by, in one process.
//   * drhip_copy_if, 2^28 u32 (x[i] < threshold, x random): selectivity 0,
//     0.01, 0.5 and 1.0, and at 0.5 both store variants of the kernel template
//     (LDS-staged 16-byte stores / per-lane stores at the ballot ranks),
//     instantiated here from dr/details/select_kernel.hpp;
//   * drhip_count_if on the same input, against drhip_reduce at the same n;
//   * drhip_inclusive_scan, 2^28 i32: the yardstick, the same look-back
//     structure moving 8 B per element.
// 3 warm-up rounds, then `reps` (default 20) timed rounds; every round runs
// every variant once (the variants alternate), HIP events on the segment's
// stream around one call; median and range.  Algorithmic bytes: 4 n + 4 count
// for copy_if, 4 n for count_if and reduce, 8 n for the scan.  Every count
// and the sum of every output are checked against a plain counting kernel.
// Then, without a bar: shp::copy_if of 2^28 u32 at selectivity 0.5 on 1 and
// on 8 segments, end to end (host clock around the blocking call).
// Build: make -C tools copy_if_bench.   Run: tools/copy_if_bench [reps] [log2n]
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
__global__ void gen_u32(uint32_t *x, size_t n, uint64_t seed) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    x[i] = (uint32_t)(mix(i, seed) >> 17);
}
// res[0] += |{x[i] < thr}| (all of x when `all`), res[1] += their sum
__global__ void ref_select(const uint32_t *x, size_t n, uint32_t thr, int all, unsigned long long *res) {
  unsigned long long c = 0, s = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    if (all || x[i] < thr) c++, s += x[i];
  atomicAdd(res, c);
  atomicAdd(res + 1, s);
}

struct LtPred {
  uint32_t s;
  __device__ __forceinline__ bool operator()(const uint32_t &v, size_t) const { return v < s; }
};

struct Stat {
  double med, lo, hi;
};
static Stat stat_of(std::vector<float> t) {
  std::sort(t.begin(), t.end());
  return {t[t.size() / 2], t.front(), t.back()};
}
constexpr int kWarm = 3;

struct Variant {
  std::string name;
  std::function<void()> call;
  double bytes = 0;
  bool copies = false;   // writes out / *count: checked against ref_select
  uint32_t thr = 0;
  int all = 0;
  std::vector<float> t;
};

int main(int argc, char **argv) {
  const int reps = argc > 1 ? std::max(1, atoi(argv[1])) : 20;
  const int log2n = argc > 2 ? atoi(argv[2]) : 28;
  const size_t n = size_t(1) << log2n;
  shp::init(std::vector<int>{0});
  hipStream_t st = shp::stream(0);
  printf("copy_if_bench: n = 2^%d, %d warm-up + %d timed rounds, every variant once per round, median (min-max), "
         "HIP events\n", log2n, kWarm, reps);

  uint32_t *x, *out;
  CK(hipMalloc(&x, n * 4));
  CK(hipMalloc(&out, n * 4));
  hipLaunchKernelGGL(gen_u32, dim3(4096), dim3(256), 0, st, x, n, 12345ull);
  unsigned long long *count, *d_ref;
  double *red;
  unsigned *err;
  CK(hipHostMalloc(&count, 8));
  CK(hipHostMalloc(&err, 4));
  *err = 0;
  CK(hipMalloc(&d_ref, 16));
  CK(hipMalloc(&red, 8));
  char *state;
  const size_t state_b = dr_select::sel_state_bytes<uint32_t>(n);
  CK(hipMalloc(&state, state_b));

  auto abi_copy = [&](int cmp, uint32_t thr) {
    return [=] { CD(drhip_copy_if(0, DRHIP_U32, cmp, x, out, n, &thr, (uint64_t *)count)); };
  };
  auto tmpl_copy = [&](auto mode, uint32_t thr) {
    return [=] {
      constexpr int MODE = decltype(mode)::value;
      CK(hipMemsetAsync(state, 0, state_b, st));
      CK((dr_select::sel_launch_span<uint32_t, MODE>(st, (const uint32_t *)x, out, n, LtPred{thr},
                                                     dr_select::sel_args{state, count, err}, 0u)));
    };
  };
  const uint32_t t001 = (uint32_t)(0.01 * 4294967296.0), t05 = 1u << 31;
  std::vector<Variant> vs;
  auto add = [&](const char *name, std::function<void()> call, bool copies, uint32_t thr, int all) {
    Variant v;
    v.name = name, v.call = call, v.copies = copies, v.thr = thr, v.all = all;
    vs.push_back(v);
  };
  add("drhip_copy_if  sel 0.00          ", abi_copy(DRHIP_LT, 0u), true, 0u, 0);
  add("drhip_copy_if  sel 0.01          ", abi_copy(DRHIP_LT, t001), true, t001, 0);
  add("drhip_copy_if  sel 0.50          ", abi_copy(DRHIP_LT, t05), true, t05, 0);
  add("template       sel 0.50 staged   ", tmpl_copy(std::integral_constant<int, dr_select::SEL_STAGED>{}, t05), true, t05, 0);
  add("template       sel 0.50 per-lane ", tmpl_copy(std::integral_constant<int, dr_select::SEL_DIRECT>{}, t05), true, t05, 0);
  // selectivity 1.0 through a real comparison (x < 0xFFFFFFFF), not a predicate the compiler folds
  add("drhip_copy_if  sel 1.00          ", abi_copy(DRHIP_LT, 0xFFFFFFFFu), true, 0xFFFFFFFFu, 0);
  add("drhip_count_if sel 0.50          ", [=] { CD(drhip_count_if(0, DRHIP_U32, DRHIP_LT, x, n, &t05, (uint64_t *)count)); },
      false, t05, 0);
  add("drhip_reduce u32 plus            ", [=] { CD(drhip_reduce(0, DRHIP_U32, DRHIP_PLUS, x, n, red)); }, false, 0u, -1);
  add("drhip_inclusive_scan i32 plus    ", [=] { CD(drhip_inclusive_scan(0, DRHIP_I32, DRHIP_PLUS, x, out, n, nullptr, nullptr, nullptr, nullptr)); },
      false, 0u, -1);

  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  std::vector<unsigned long long> got_count(vs.size(), 0);
  for (int r = -kWarm; r < reps; r++)
    for (size_t i = 0; i < vs.size(); i++) {
      CK(hipEventRecord(e0, st));
      vs[i].call();
      CK(hipEventRecord(e1, st));
      CK(hipStreamSynchronize(st));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= 0) vs[i].t.push_back(ms);
      got_count[i] = *count;
    }
  if (*err) printf("ERROR: the kernel's error word is %u\n", *err);

  // checks (outside the timing): the count of every selecting variant, and the sum of a fresh output
  int bad = 0;
  double scan_ms = 0, reduce_ms = 0, worst_copy = 0, count_ms = 0;
  for (size_t i = 0; i < vs.size(); i++) {
    Variant &v = vs[i];
    const Stat s = stat_of(v.t);
    unsigned long long c = 0;
    const char *ok = "";
    if (v.all >= 0) {
      unsigned long long ref[2];
      CK(hipMemsetAsync(d_ref, 0, 16, st));
      hipLaunchKernelGGL(ref_select, dim3(2048), dim3(256), 0, st, x, n, v.thr, v.all, d_ref);
      CK(hipMemcpyAsync(ref, d_ref, 16, hipMemcpyDeviceToHost, st));
      CK(hipStreamSynchronize(st));
      c = got_count[i];
      bool good = c == ref[0];
      if (v.copies && good) {
        v.call(); // a fresh output, then its sum
        CK(hipStreamSynchronize(st));
        unsigned long long sum[2];
        CK(hipMemsetAsync(d_ref, 0, 16, st));
        hipLaunchKernelGGL(ref_select, dim3(2048), dim3(256), 0, st, out, (size_t)c, 0u, 1, d_ref);
        CK(hipMemcpyAsync(sum, d_ref, 16, hipMemcpyDeviceToHost, st));
        CK(hipStreamSynchronize(st));
        good = sum[1] == ref[1];
      }
      ok = good ? "  ok" : "  WRONG";
      bad += !good;
    }
    const bool is_scan = v.name.find("scan") != std::string::npos, is_red = v.name.find("reduce") != std::string::npos;
    v.bytes = is_scan ? 8.0 * n : v.copies ? 4.0 * n + 4.0 * c : 4.0 * n;
    if (is_scan) scan_ms = s.med;
    if (is_red) reduce_ms = s.med;
    if (v.name.find("drhip_copy_if") == 0) worst_copy = std::max(worst_copy, s.med);
    if (v.name.find("drhip_count_if") == 0) count_ms = s.med;
    printf("%s %8.3f ms (%.3f-%.3f)  %12.0f B  %7.1f GB/s", v.name.c_str(), s.med, s.lo, s.hi, v.bytes,
           v.bytes / s.med / 1e6);
    if (v.all >= 0) printf("  count=%llu%s", c, ok);
    printf("\n");
  }
  printf("bar copy_if : slowest drhip_copy_if %.3f ms vs scan %.3f ms x 1.15 = %.3f ms: %s\n", worst_copy, scan_ms,
         scan_ms * 1.15, worst_copy <= scan_ms * 1.15 ? "met" : "MISSED");
  printf("bar count_if: %.3f ms vs drhip_reduce %.3f ms x 1.15 = %.3f ms: %s\n", count_ms, reduce_ms, reduce_ms * 1.15,
         count_ms <= reduce_ms * 1.15 ? "met" : "MISSED");
  fflush(stdout);
  CK(hipFree(x));
  CK(hipFree(out));
  CK(hipFree(d_ref));
  CK(hipFree(red));
  CK(hipFree(state));
  CK(hipHostFree(count));
  CK(hipHostFree(err));
  shp::finalize();

  // shp::copy_if end to end, 1 and 8 segments (duplicated on the visible devices)
  for (std::size_t segs : {std::size_t(1), std::size_t(8)}) {
    shp::init(shp::get_duplicated_devices(shp::get_numa_devices(), segs));
    {
      shp::distributed_vector<uint32_t> in(n), o(n);
      for (auto &s : in.segments())
        hipLaunchKernelGGL(gen_u32, dim3(4096), dim3(256), 0, shp::stream(s.rank()), s.data(), s.size(),
                           777ull + s.rank());
      shp::sync_all();
      const uint32_t thr = t05;
      auto pred = [thr] __device__(uint32_t v) { return v < thr; };
      std::vector<double> t;
      std::size_t got = 0;
      const int r2 = std::min(reps, 10);
      for (int r = -kWarm; r < r2; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        auto it = shp::copy_if(shp::par_unseq, in, o, pred);
        const auto t1 = std::chrono::steady_clock::now();
        got = (std::size_t)(it - o.begin());
        if (r >= 0) t.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
      }
      std::sort(t.begin(), t.end());
      const std::size_t cnt = shp::count_if(shp::par_unseq, in, pred);
      printf("shp::copy_if n=2^%d sel 0.50, %zu segment%s on %zu device%s, end to end: %8.3f ms (%.3f-%.3f)  copied=%zu%s\n",
             log2n, segs, segs > 1 ? "s" : "", (std::size_t)std::min<std::size_t>(segs, shp::get_numa_devices().size()),
             segs > 1 && shp::get_numa_devices().size() > 1 ? "s" : "", t[t.size() / 2], t.front(), t.back(), got,
             got == cnt ? "  ok" : "  WRONG");
      bad += got != cnt;
    }
    shp::finalize();
  }
  return bad ? 1 : 0;
}
