// scan_by_key_bench.hip -- measurement tool (not product): times the by-key
// scans of the C-ABI on ONE device against the entry points they are judged
// by, in one process and at one n.
//   * drhip_inclusive_scan_by_key and drhip_exclusive_scan_by_key (init 5),
//     2^28 u32 keys + u32 values, PLUS: run lengths 1, 4, 32, 1024 and all
//     keys equal (keys[i] = i / L); 12 B move per element;
//   * the same kernel template with 16 slots per thread instead of the shipped
//     8 (twice the tile), run length 1024 and all equal: the tile-shape
//     comparison;
//   * the yardsticks: drhip_inclusive_scan of 2^28 u32 (the look-back scan,
//     8 B per element) and drhip_reduce_by_key at the same run lengths.
// Goal: at run length 1024 and at all-equal at most 1.5 x the look-back scan's
// time plus 15 %, and no slower than reduce_by_key at the same run length.
// 3 warm-up rounds, then `reps` (default 20) timed rounds; every round runs
// every variant once (the variants alternate); a variant's keys are generated
// on the stream before the first event, so they are not timed; HIP events
// around one call; median and range.  Every variant's output is checked by
// its sum (a fresh call, outside the timing): with keys i / L and values
// v[i] the sum of the inclusive scan is sum_i v[i] * (L - i % L) (cut at n),
// computed by a kernel of its own from the inputs.
// Then, without a bar: shp::inclusive_scan_by_key of 2^28 u32/u32 pairs, run
// length 1024, on 1 and on 8 segments, end to end (host clock around the
// blocking call).
// Build: make -C tools scan_by_key_bench.   Run: tools/scan_by_key_bench [reps] [log2n]
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
// keys[i] = (i0 + i) / L (L == 0: all equal)
__global__ void gen_keys(uint32_t *k, size_t n, size_t L, size_t i0) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    k[i] = L ? (uint32_t)((i0 + i) / L) : 7u;
}
__global__ void gen_vals(uint32_t *v, size_t n, uint64_t seed) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    v[i] = (uint32_t)(mix(i, seed) & 7);
}
// *res += the sum of x[0, n) modulo 2^64
__global__ void sum_of(const uint32_t *x, size_t n, unsigned long long *res) {
  unsigned long long s = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) s += x[i];
  atomicAdd(res, s);
}
// *res += what the scan's outputs must sum to (L == 0: one run of n): element i is counted by every element from
// itself (inclusive) or from its successor (exclusive) to the end of its run; every element adds init (exclusive)
__global__ void want_sum(const uint32_t *v, size_t n, size_t L, int excl, unsigned long long init, unsigned long long *res) {
  unsigned long long s = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    size_t end = L ? (i / L + 1) * L : n;
    if (end > n) end = n;
    s += (unsigned long long)v[i] * (end - i - (excl ? 1 : 0)) + (excl ? init : 0);
  }
  atomicAdd(res, s);
}

struct KeyEqU32 {
  __device__ __forceinline__ bool operator()(const uint32_t &a, const uint32_t &b) const { return a == b; }
};
struct PlusU32 {
  __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
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
  std::function<void()> prep, call;
  double bytes = 0;
  int kind = 0; // 0: not checked here, 1: inclusive by key, 2: exclusive by key
  size_t L = 0;
  std::vector<float> t;
};

int main(int argc, char **argv) {
  const int reps = argc > 1 ? std::max(1, atoi(argv[1])) : 20;
  const int log2n = argc > 2 ? atoi(argv[2]) : 28;
  const size_t n = size_t(1) << log2n;
  shp::init(std::vector<int>{0});
  hipStream_t st = shp::stream(0);
  printf("scan_by_key_bench: n = 2^%d u32 keys + u32 values, PLUS, %d warm-up + %d timed rounds, every variant once per round, "
         "median (min-max), HIP events\n", log2n, kWarm, reps);

  uint32_t *kin, *vin, *kout, *vout;
  CK(hipMalloc(&kin, n * 4));
  CK(hipMalloc(&vin, n * 4));
  CK(hipMalloc(&kout, n * 4));
  CK(hipMalloc(&vout, n * 4));
  unsigned long long *count, *d_sum;
  CK(hipHostMalloc(&count, 8));
  CK(hipMalloc(&d_sum, 8));
  hipLaunchKernelGGL(gen_vals, dim3(4096), dim3(256), 0, st, vin, n, 99ull);
  const uint32_t init = 5;

  std::vector<Variant> vs;
  auto add = [&](std::string name, std::function<void()> prep, std::function<void()> call, int kind, size_t L, double bytes) {
    Variant v;
    v.name = name, v.prep = prep, v.call = call, v.kind = kind, v.L = L, v.bytes = bytes;
    vs.push_back(v);
  };
  auto prep = [&](size_t L) {
    return [=] { hipLaunchKernelGGL(gen_keys, dim3(4096), dim3(256), 0, st, kin, n, L, (size_t)0); };
  };
  auto runs_of = [&](size_t L) { return L ? (n + L - 1) / L : (size_t)1; };
  auto incl = [=] { CD(drhip_inclusive_scan_by_key(0, DRHIP_U32, DRHIP_U32, DRHIP_PLUS, kin, vin, n, vout)); };
  auto excl = [=] { CD(drhip_exclusive_scan_by_key(0, DRHIP_U32, DRHIP_U32, DRHIP_PLUS, kin, vin, n, &init, vout)); };
  auto rbk = [=] { CD(drhip_reduce_by_key(0, DRHIP_U32, DRHIP_U32, DRHIP_PLUS, kin, vin, n, kout, vout, (uint64_t *)count)); };
  unsigned *err;
  CK(hipHostMalloc(&err, 4));
  *err = 0;
  char *state;
  CK(hipMalloc(&state, dr_segscan::ss_state_bytes(dr_segreduce::sr_tiles<uint32_t, uint32_t, true>(n))));
  auto incl_u16 = [=] {
    CK((dr_segscan::ss_launch<uint32_t, uint32_t, uint32_t, true, false, 16>(st, (const uint32_t *)kin, (const uint32_t *)vin, n, vout,
                                                                              0u, KeyEqU32{}, PlusU32{},
                                                                              dr_segscan::ss_args{state, err})));
  };
  const size_t Ls[] = {1, 4, 32, 1024, 0};
  auto label = [](size_t L) { return L ? "run " + std::to_string(L) : std::string("all equal"); };
  auto pad = [](std::string s) {
    s.resize(40, ' ');
    return s;
  };

  add(pad("drhip_inclusive_scan u32 (yardstick)"), [] {},
      [=] { CD(drhip_inclusive_scan(0, DRHIP_U32, DRHIP_PLUS, vin, vout, n, nullptr, nullptr, nullptr, nullptr)); }, 0, 0, 8.0 * n);
  for (size_t L : Ls) add(pad("inclusive_scan_by_key " + label(L)), prep(L), incl, 1, L, 12.0 * n);
  for (size_t L : Ls) add(pad("exclusive_scan_by_key " + label(L)), prep(L), excl, 2, L, 12.0 * n);
  for (size_t L : {size_t(1024), size_t(0)}) add(pad("template 16 slots incl. " + label(L)), prep(L), incl_u16, 1, L, 12.0 * n);
  for (size_t L : Ls) add(pad("reduce_by_key " + label(L)), prep(L), rbk, 0, L, 8.0 * n + 8.0 * runs_of(L));

  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int r = -kWarm; r < reps; r++)
    for (auto &v : vs) {
      v.prep();
      CK(hipEventRecord(e0, st));
      v.call();
      CK(hipEventRecord(e1, st));
      CK(hipStreamSynchronize(st));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= 0) v.t.push_back(ms);
    }
  CD(drhip_sync(0)); // the look-backs' error word
  if (*err) printf("ERROR: the template launches' error word is %u\n", *err);

  auto fetch = [&] {
    unsigned long long s = 0;
    CK(hipMemcpyAsync(&s, d_sum, 8, hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    return s;
  };
  int bad = 0;
  std::vector<double> med(vs.size());
  for (size_t i = 0; i < vs.size(); i++) {
    Variant &v = vs[i];
    const Stat s = stat_of(v.t);
    med[i] = s.med;
    std::string ok;
    if (v.kind) {
      v.prep();
      CK(hipMemsetAsync(vout, 0xA5, n * 4, st));
      v.call();
      CK(hipMemsetAsync(d_sum, 0, 8, st));
      // the outputs wrap modulo 2^32 only where a run's sum passes 2^32: 7 * 2^28 does not
      hipLaunchKernelGGL(sum_of, dim3(2048), dim3(256), 0, st, vout, n, d_sum);
      const unsigned long long got = fetch();
      CK(hipMemsetAsync(d_sum, 0, 8, st));
      hipLaunchKernelGGL(want_sum, dim3(2048), dim3(256), 0, st, vin, n, v.L, v.kind == 2 ? 1 : 0, (unsigned long long)init, d_sum);
      const unsigned long long want = fetch();
      const bool good = got == want;
      ok = good ? "  ok" : "  WRONG";
      bad += !good;
    }
    printf("%s %8.3f ms (%.3f-%.3f)  %12.0f B  %7.1f GB/s%s\n", v.name.c_str(), s.med, s.lo, s.hi, v.bytes, v.bytes / s.med / 1e6,
           ok.c_str());
  }
  auto ms_of = [&](const std::string &prefix) {
    for (size_t i = 0; i < vs.size(); i++)
      if (vs[i].name.find(prefix) == 0 && (vs[i].name.size() == prefix.size() || vs[i].name[prefix.size()] == ' ')) return med[i];
    return 0.0;
  };
  const double scan = ms_of("drhip_inclusive_scan u32 (yardstick)"), bar = scan * 1.5 * 1.15;
  for (const char *form : {"inclusive_scan_by_key ", "exclusive_scan_by_key "})
    for (size_t L : {size_t(1024), size_t(0)}) {
      const double t = ms_of(form + label(L)), r = ms_of("reduce_by_key " + label(L));
      printf("goal %s%-9s: %.3f ms = %.2f x the look-back scan's %.3f ms (goal: at most 1.5 x 1.15 = 1.725 x = %.3f ms): %s; "
             "%.2f x reduce_by_key's %.3f ms: %s\n",
             form, label(L).c_str(), t, t / scan, scan, bar, t <= bar ? "met" : "MISSED", t / r, r, t <= r ? "met" : "MISSED");
    }
  fflush(stdout);
  for (void *p : {(void *)kin, (void *)vin, (void *)kout, (void *)vout, (void *)d_sum, (void *)state}) CK(hipFree(p));
  CK(hipHostFree(err));
  CK(hipHostFree(count));
  shp::finalize();

  // shp::inclusive_scan_by_key end to end, 1 and 8 segments (duplicated on the visible devices)
  for (std::size_t segs : {std::size_t(1), std::size_t(8)}) {
    shp::init(shp::get_duplicated_devices(shp::get_numa_devices(), segs));
    {
      shp::distributed_vector<uint32_t> k(n), v(n), o(n);
      std::size_t i0 = 0;
      for (auto &s : k.segments()) {
        hipLaunchKernelGGL(gen_keys, dim3(4096), dim3(256), 0, shp::stream(s.rank()), s.data(), s.size(), (size_t)1024, i0);
        i0 += s.size();
      }
      for (auto &s : v.segments())
        hipLaunchKernelGGL(gen_vals, dim3(4096), dim3(256), 0, shp::stream(s.rank()), s.data(), s.size(), 777ull + s.rank());
      shp::sync_all();
      std::vector<double> t;
      const int r2 = std::min(reps, 10);
      for (int r = -kWarm; r < r2; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        shp::inclusive_scan_by_key(shp::par_unseq, k, v, o);
        const auto t1 = std::chrono::steady_clock::now();
        if (r >= 0) t.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
      }
      std::sort(t.begin(), t.end());
      // the last elements of the runs are the runs' sums: their total is the values' total
      std::vector<uint32_t> ho(n), hv(n);
      shp::copy(o.begin(), o.end(), ho.begin());
      shp::copy(v.begin(), v.end(), hv.begin());
      unsigned long long so = 0, sv = 0;
      for (std::size_t i = 0; i < n; i++) {
        sv += hv[i];
        if (i % 1024 == 1023 || i == n - 1) so += ho[i];
      }
      const bool good = so == sv;
      printf("shp::inclusive_scan_by_key n=2^%d run 1024, %zu segment%s on %zu device%s, end to end: %8.3f ms (%.3f-%.3f)%s\n", log2n,
             segs, segs > 1 ? "s" : "", (std::size_t)std::min<std::size_t>(segs, shp::get_numa_devices().size()),
             segs > 1 && shp::get_numa_devices().size() > 1 ? "s" : "", t[t.size() / 2], t.front(), t.back(), good ? "  ok" : "  WRONG");
      bad += !good;
    }
    shp::finalize();
  }
  return bad ? 1 : 0;
}
