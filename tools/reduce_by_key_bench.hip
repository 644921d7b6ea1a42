// reduce_by_key_bench.hip -- measurement tool (not product): times the by-key
// reduction C-ABI on ONE device against the entry points it is judged by, in
// one process.
//   * drhip_reduce_by_key, 2^28 u32 keys + u32 values, PLUS: run lengths 1, 4,
//     32, 1024 and all keys equal (keys[i] = i / L);
//   * the same kernel template with 4 slots per thread instead of the shipped
//     8 (half the tile), run lengths 4 and 1024: the tile-shape comparison;
//   * u64 keys with f64 values at 2^27, run lengths 4 and 1024;
//   * drhip_run_length_encode (run length 1024) and drhip_unique_copy (run
//     lengths 1 and 1024), the latter beside drhip_copy_if at selectivity 1.0
//     and 1/1024, and beside selection's template with the predicate
//     (x, i) -> i == 0 || in[i-1] != x, the other way to build it;
//   * the yardsticks: drhip_dot of 2^28 u32 pairs (the same 8 n bytes from two
//     streams) and drhip_copy_if at selectivity 1.0 (twice that moves keys and
//     values through the nearest existing kernel).
// 3 warm-up rounds, then `reps` (default 20) timed rounds; every round runs
// every variant once (the variants alternate); a variant's keys are generated
// on the stream before the first event, so they are not timed; HIP events
// around one call; median and range.  Every run count and the sums of the
// output keys and values are checked (a fresh call, outside the timing).
// Then, without a bar: shp::reduce_by_key of 2^28 u32/u32 pairs, run length
// 1024, on 1 and on 8 segments, end to end (host clock around the blocking call).
// Build: make -C tools reduce_by_key_bench.   Run: tools/reduce_by_key_bench [reps] [log2n]
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
template <typename K> __global__ void gen_keys(K *k, size_t n, size_t L, size_t i0) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    k[i] = L ? (K)((i0 + i) / L) : (K)7;
}
template <typename V> __global__ void gen_vals(V *v, size_t n, uint64_t seed) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    v[i] = (V)(mix(i, seed) & 7);
}
__global__ void gen_u32(uint32_t *x, size_t n, uint64_t seed) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    x[i] = (uint32_t)(mix(i, seed) >> 17);
}
// *res += the sum of x[0, n) as uint64 (the values are small whole numbers)
template <typename T> __global__ void sum_of(const T *x, size_t n, unsigned long long *res) {
  unsigned long long s = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    s += (unsigned long long)x[i];
  atomicAdd(res, s);
}

template <typename K> struct KeyEq {
  __device__ __forceinline__ bool operator()(const K &a, const K &b) const { return a == b; }
};
// unique_copy's other form: selection's template with "differs from its predecessor" as the predicate
struct NeighbourPred {
  const uint32_t *in;
  __device__ __forceinline__ bool operator()(const uint32_t &x, size_t i) const { return i == 0 || in[i - 1] != x; }
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
  // checks: kind 0 none, 1 keys + values (u32), 2 keys + values (u64 / f64), 3 keys (u32) + counts (u64), 4 keys only (u32)
  int kind = 0;
  size_t n = 0, L = 0;
  std::vector<float> t;
};

int main(int argc, char **argv) {
  const int reps = argc > 1 ? std::max(1, atoi(argv[1])) : 20;
  const int log2n = argc > 2 ? atoi(argv[2]) : 28;
  const size_t n = size_t(1) << log2n, n8 = n / 2;
  shp::init(std::vector<int>{0});
  hipStream_t st = shp::stream(0);
  printf("reduce_by_key_bench: n = 2^%d (u64/f64: 2^%d), %d warm-up + %d timed rounds, every variant once per round, "
         "median (min-max), HIP events\n", log2n, log2n - 1, kWarm, reps);

  // four buffers of 4 n bytes: keys, values, keys out, values out (counts out: 8 n / 2 ... the u64 variants use n / 2)
  void *kin, *vin, *kout, *vout;
  CK(hipMalloc(&kin, n * 4));
  CK(hipMalloc(&vin, n * 4));
  CK(hipMalloc(&kout, n * 4));
  CK(hipMalloc(&vout, n * 8)); // run_length_encode of n u32 keys may write n uint64 counts
  uint32_t *x;                 // the yardsticks' random input
  CK(hipMalloc(&x, n * 4));
  hipLaunchKernelGGL(gen_u32, dim3(4096), dim3(256), 0, st, x, n, 12345ull);
  unsigned long long *count, *d_sum;
  unsigned *err;
  double *red;
  CK(hipHostMalloc(&count, 8));
  CK(hipHostMalloc(&err, 4));
  *err = 0;
  CK(hipMalloc(&d_sum, 8));
  CK(hipMalloc(&red, 8));
  char *state;
  const size_t state_b = std::max(dr_segreduce::sr_state_bytes(dr_segreduce::sr_tiles<uint32_t, uint32_t, true, 4>(n)),
                                  dr_select::sel_state_bytes<uint32_t>(n));
  CK(hipMalloc(&state, state_b));

  std::vector<Variant> vs;
  auto add = [&](const char *name, std::function<void()> prep, std::function<void()> call, int kind, size_t vn, size_t L,
                 double bytes) {
    Variant v;
    v.name = name, v.prep = prep, v.call = call, v.kind = kind, v.n = vn, v.L = L, v.bytes = bytes;
    vs.push_back(v);
  };
  auto runs_of = [](size_t vn, size_t L) { return L ? (vn + L - 1) / L : (size_t)1; };
  auto prep32 = [&](size_t L) {
    return [=] {
      hipLaunchKernelGGL(gen_keys<uint32_t>, dim3(4096), dim3(256), 0, st, (uint32_t *)kin, n, L, (size_t)0);
      hipLaunchKernelGGL(gen_vals<uint32_t>, dim3(4096), dim3(256), 0, st, (uint32_t *)vin, n, 99ull);
    };
  };
  auto prep64 = [&](size_t L) {
    return [=] {
      hipLaunchKernelGGL(gen_keys<uint64_t>, dim3(4096), dim3(256), 0, st, (uint64_t *)kin, n8, L, (size_t)0);
      hipLaunchKernelGGL(gen_vals<double>, dim3(4096), dim3(256), 0, st, (double *)vin, n8, 99ull);
    };
  };
  auto rbk32 = [=] { CD(drhip_reduce_by_key(0, DRHIP_U32, DRHIP_U32, DRHIP_PLUS, kin, vin, n, kout, vout, (uint64_t *)count)); };
  auto rbk64 = [=] { CD(drhip_reduce_by_key(0, DRHIP_U64, DRHIP_F64, DRHIP_PLUS, kin, vin, n8, kout, vout, (uint64_t *)count)); };
  auto rbk32_u4 = [=] {
    CK((dr_segreduce::sr_launch<uint32_t, uint32_t, uint32_t, true, true, 4>(
        st, (const uint32_t *)kin, (const uint32_t *)vin, n, (uint32_t *)kout, (uint32_t *)vout, KeyEq<uint32_t>{}, PlusU32{},
        dr_segreduce::sr_args{state, count, err})));
  };
  auto uniq_select = [=] {
    CK(hipMemsetAsync(state, 0, dr_select::sel_state_bytes<uint32_t>(n), st));
    CK((dr_select::sel_launch_span<uint32_t, dr_select::kSelMode>(st, (const uint32_t *)kin, (uint32_t *)kout, n,
                                                                  NeighbourPred{(const uint32_t *)kin},
                                                                  dr_select::sel_args{state, count, err}, 0u)));
  };
  auto b32 = [&](size_t L) { return 8.0 * n + 8.0 * runs_of(n, L); };
  auto b64 = [&](size_t L) { return 16.0 * n8 + 16.0 * runs_of(n8, L); };
  const uint32_t all = 0xFFFFFFFFu, t1024 = 1u << 22;

  add("drhip_dot u32 (yardstick)          ", [] {}, [=] { CD(drhip_dot(0, DRHIP_U32, x, vin, n, red)); }, 0, n, 0, 8.0 * n);
  add("drhip_copy_if sel 1.00 (yardstick) ", [] {},
      [=] { CD(drhip_copy_if(0, DRHIP_U32, DRHIP_LT, x, kout, n, &all, (uint64_t *)count)); }, 0, n, 0, 8.0 * n);
  add("drhip_copy_if sel 1/1024           ", [] {},
      [=] { CD(drhip_copy_if(0, DRHIP_U32, DRHIP_LT, x, kout, n, &t1024, (uint64_t *)count)); }, 0, n, 0, 4.0 * n + 4.0 * n / 1024);
  add("reduce_by_key u32/u32 run 1        ", prep32(1), rbk32, 1, n, 1, b32(1));
  add("reduce_by_key u32/u32 run 4        ", prep32(4), rbk32, 1, n, 4, b32(4));
  add("reduce_by_key u32/u32 run 32       ", prep32(32), rbk32, 1, n, 32, b32(32));
  add("reduce_by_key u32/u32 run 1024     ", prep32(1024), rbk32, 1, n, 1024, b32(1024));
  add("reduce_by_key u32/u32 all equal    ", prep32(0), rbk32, 1, n, 0, b32(0));
  add("template 4 slots u32/u32 run 4     ", prep32(4), rbk32_u4, 1, n, 4, b32(4));
  add("template 4 slots u32/u32 run 1024  ", prep32(1024), rbk32_u4, 1, n, 1024, b32(1024));
  add("reduce_by_key u64/f64 run 4        ", prep64(4), rbk64, 2, n8, 4, b64(4));
  add("reduce_by_key u64/f64 run 1024     ", prep64(1024), rbk64, 2, n8, 1024, b64(1024));
  add("run_length_encode u32 run 1024     ", prep32(1024),
      [=] { CD(drhip_run_length_encode(0, DRHIP_U32, kin, n, kout, (uint64_t *)vout, (uint64_t *)count)); }, 3, n, 1024,
      4.0 * n + 12.0 * runs_of(n, 1024));
  add("unique_copy u32 run 1              ", prep32(1), [=] { CD(drhip_unique_copy(0, DRHIP_U32, kin, n, kout, (uint64_t *)count)); },
      4, n, 1, 8.0 * n);
  add("unique_copy u32 run 1024           ", prep32(1024),
      [=] { CD(drhip_unique_copy(0, DRHIP_U32, kin, n, kout, (uint64_t *)count)); }, 4, n, 1024, 4.0 * n + 4.0 * runs_of(n, 1024));

  add("select template, neighbour pred 1  ", prep32(1), uniq_select, 4, n, 1, 8.0 * n);
  add("select template, neighbour pred 1024", prep32(1024), uniq_select, 4, n, 1024, 4.0 * n + 4.0 * runs_of(n, 1024));

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
  if (*err) printf("ERROR: the kernel's error word is %u\n", *err);

  // checks (outside the timing): a fresh call, its run count, the sums of its keys and values
  auto sum_dev = [&](auto *p, size_t m) {
    unsigned long long s = 0;
    CK(hipMemsetAsync(d_sum, 0, 8, st));
    hipLaunchKernelGGL(sum_of<std::remove_pointer_t<decltype(p)>>, dim3(2048), dim3(256), 0, st, p, m, d_sum);
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
      *count = ~0ull;
      v.call();
      CK(hipStreamSynchronize(st));
      const size_t runs = runs_of(v.n, v.L), c = (size_t)*count;
      bool good = c == runs;
      if (good) {
        // keys: 0, 1, ..., runs - 1 (all equal: the one key 7)
        const unsigned long long want_k = v.L ? (unsigned long long)runs * (runs - 1) / 2 : 7ull;
        const unsigned long long got_k = v.kind == 2 ? sum_dev((const uint64_t *)kout, c) : sum_dev((const uint32_t *)kout, c);
        good = got_k == want_k;
        if (v.kind == 1) { // u32 sums wrap per run; the total agrees modulo 2^32
          good = good && (uint32_t)sum_dev((const uint32_t *)vout, c) == (uint32_t)sum_dev((const uint32_t *)vin, v.n);
        } else if (v.kind == 2) {
          good = good && sum_dev((const double *)vout, c) == sum_dev((const double *)vin, v.n);
        } else if (v.kind == 3) {
          good = good && sum_dev((const uint64_t *)vout, c) == v.n;
        }
      }
      ok = "  runs=" + std::to_string(c) + (good ? "  ok" : "  WRONG");
      bad += !good;
    }
    printf("%s %8.3f ms (%.3f-%.3f)  %12.0f B  %7.1f GB/s%s\n", v.name.c_str(), s.med, s.lo, s.hi, v.bytes, v.bytes / s.med / 1e6,
           ok.c_str());
  }
  auto ms_of = [&](const char *prefix) {
    for (size_t i = 0; i < vs.size(); i++)
      if (vs[i].name.find(prefix) == 0) return med[i];
    return 0.0;
  };
  const double dot = ms_of("drhip_dot"), r1024 = ms_of("reduce_by_key u32/u32 run 1024"), r1 = ms_of("reduce_by_key u32/u32 run 1 "),
               eq = ms_of("reduce_by_key u32/u32 all equal"), c1 = ms_of("drhip_copy_if sel 1.00");
  printf("bar long runs : run 1024 %.3f ms vs drhip_dot %.3f ms x 1.75 = %.3f ms: %s\n", r1024, dot, dot * 1.75,
         r1024 <= dot * 1.75 ? "met" : "MISSED");
  printf("bar all equal : %.3f ms vs run 1024 %.3f ms x 1.5 = %.3f ms: %s\n", eq, r1024, r1024 * 1.5,
         eq <= r1024 * 1.5 ? "met" : "MISSED");
  printf("no bar        : run 1 %.3f ms beside 2 x drhip_copy_if sel 1.00 = %.3f ms\n", r1, 2 * c1);
  fflush(stdout);
  for (void *p : {kin, vin, kout, vout, (void *)x, (void *)d_sum, (void *)red, (void *)state}) CK(hipFree(p));
  CK(hipHostFree(count));
  CK(hipHostFree(err));
  shp::finalize();

  // shp::reduce_by_key end to end, 1 and 8 segments (duplicated on the visible devices)
  for (std::size_t segs : {std::size_t(1), std::size_t(8)}) {
    shp::init(shp::get_duplicated_devices(shp::get_numa_devices(), segs));
    {
      shp::distributed_vector<uint32_t> k(n), v(n), ok(n), ov(n);
      std::size_t i0 = 0;
      for (auto &s : k.segments()) {
        hipLaunchKernelGGL(gen_keys<uint32_t>, dim3(4096), dim3(256), 0, shp::stream(s.rank()), s.data(), s.size(), (size_t)1024, i0);
        i0 += s.size();
      }
      for (auto &s : v.segments())
        hipLaunchKernelGGL(gen_vals<uint32_t>, dim3(4096), dim3(256), 0, shp::stream(s.rank()), s.data(), s.size(), 777ull + s.rank());
      shp::sync_all();
      std::vector<double> t;
      std::size_t got = 0;
      const int r2 = std::min(reps, 10);
      for (int r = -kWarm; r < r2; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        auto [ik, iv] = shp::reduce_by_key(shp::par_unseq, k, v, ok, ov);
        const auto t1 = std::chrono::steady_clock::now();
        got = (std::size_t)(ik - ok.begin());
        if (r >= 0) t.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
      }
      std::sort(t.begin(), t.end());
      const std::size_t want = (n + 1023) / 1024;
      const uint32_t sv = shp::reduce(shp::par_unseq, v, uint32_t(0), std::plus<>{});
      const uint32_t so = shp::reduce(shp::par_unseq, ov | shp::views::take(got), uint32_t(0), std::plus<>{});
      const bool good = got == want && sv == so;
      printf("shp::reduce_by_key n=2^%d run 1024, %zu segment%s on %zu device%s, end to end: %8.3f ms (%.3f-%.3f)  runs=%zu%s\n",
             log2n, segs, segs > 1 ? "s" : "", (std::size_t)std::min<std::size_t>(segs, shp::get_numa_devices().size()),
             segs > 1 && shp::get_numa_devices().size() > 1 ? "s" : "", t[t.size() / 2], t.front(), t.back(), got,
             good ? "  ok" : "  WRONG");
      bad += !good;
    }
    shp::finalize();
  }
  return bad ? 1 : 0;
}
