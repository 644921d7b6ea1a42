// merge_bench.hip -- measurement tool (not product): times drhip_merge and
// drhip_merge_pairs on ONE device against rocprim::merge (the yardstick, as
// rocPRIM's binary search is for tools/sorted_search_bench.hip), in one process
// on the same buffers.
//   rows (every input sorted): u32 and u64, 2^log2n + 2^log2n random keys;
//   u32: a entirely below b; all keys equal; 2^log2n + 2^20 (unbalanced);
//   drhip_merge_pairs, u32 keys with u32 and with u64 values, against
//   rocprim::merge with values.
// Per row: 2 warm-up rounds, then `reps` (default 10) timed rounds; every round
// runs both implementations once (they alternate), HIP events on the segment's
// stream around one call; the median per implementation is printed, in
// microseconds, with the least and the greatest round.  The two outputs are
// compared element by element.  Run the tool at least three times: the bar
// (drhip's median no slower than rocPRIM's by more than the larger run-to-run
// spread) is judged across process runs.
// For information: drhip_inclusive_scan of 2^(log2n + 1) u32, the in-project
// yardstick that moves the same 8 B per output element; shp::merge end to end
// on 1 and on 8 segments of the visible devices.
// --sweep: the kernel of drhip_merge with 4 / 8 / 16 items per thread (tiles of
// 1024 / 2048 / 4096) and 2 / 4 / 8 workgroups per CU, random keys.
// Build: make -C tools merge_bench.
// Run: tools/merge_bench [reps] [log2n] [--sweep]
#include <dr/shp.hpp>

#include <rocprim/device/device_merge.hpp>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

__host__ __device__ inline uint64_t mix(uint64_t i, uint64_t seed) {
  uint64_t h = (i + 1) * 0x9E3779B97F4A7C15ull ^ seed;
  h ^= h >> 31;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 29;
  h *= 0x94D049BB133111EBull;
  h ^= h >> 32;
  return h;
}
template <typename T> __global__ void gen_random(T *x, size_t m, uint64_t seed) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x)
    x[i] = (T)mix(i, seed);
}
// x[i] = base + i / rep: sorted; rep = 0: all equal to base
template <typename T> __global__ void gen_ramp(T *x, size_t m, T base, size_t rep) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x)
    x[i] = rep ? (T)(base + i / rep) : base;
}
template <typename T> __global__ void gen_iota(T *x, size_t m, T base) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x) x[i] = (T)(base + i);
}
template <typename T> __global__ void count_diff(const T *a, const T *b, size_t m, unsigned long long *bad) {
  unsigned long long c = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x) c += a[i] != b[i];
  if (c) atomicAdd(bad, c);
}
// out[i - 1] <= out[i] everywhere
template <typename T> __global__ void count_descents(const T *x, size_t m, unsigned long long *bad) {
  unsigned long long c = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x + 1; i < m; i += (size_t)gridDim.x * blockDim.x) c += x[i] < x[i - 1];
  if (c) atomicAdd(bad, c);
}

template <typename T> constexpr int dtype_of() { return sizeof(T) == 4 ? DRHIP_U32 : DRHIP_U64; }
template <typename T> constexpr const char *name_of() { return sizeof(T) == 4 ? "u32" : "u64"; }

struct Stat {
  double med, lo, hi;
};
static Stat stat_of(std::vector<float> &t) {
  std::sort(t.begin(), t.end());
  return {t[t.size() / 2], t.front(), t.back()};
}

static int g_bad = 0;
static void *g_tmp = nullptr;
static size_t g_tmp_bytes = 0;
static unsigned long long *g_badw = nullptr;

template <typename T> static void sort_random(hipStream_t st, T *scratch, T *x, size_t n, uint64_t seed) {
  hipLaunchKernelGGL(gen_random<T>, dim3(4096), dim3(256), 0, st, scratch, n, seed);
  size_t sb = g_tmp_bytes;
  CK(rocprim::radix_sort_keys(g_tmp, sb, scratch, x, n, 0, sizeof(T) * 8, st));
}

// one row: drhip_merge[_pairs] against rocprim::merge; V = char: no values
template <typename T, typename V>
static void row(hipStream_t st, int reps, const char *what, const T *a, size_t na, const T *b, size_t nb, T *out_d, T *out_r,
                const V *va, const V *vb, V *vout_d, V *vout_r) {
  constexpr bool VALS = sizeof(V) > 1;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  std::vector<float> td, tr;
  for (int r = -2; r < reps; r++) {
    float ms;
    CK(hipEventRecord(e0, st));
    if constexpr (VALS) CD(drhip_merge_pairs(0, dtype_of<T>(), a, va, na, b, vb, nb, sizeof(V), out_d, vout_d));
    else CD(drhip_merge(0, dtype_of<T>(), a, na, b, nb, out_d));
    CK(hipEventRecord(e1, st));
    CK(hipStreamSynchronize(st));
    CK(hipEventElapsedTime(&ms, e0, e1));
    if (r >= 0) td.push_back(ms * 1000.f);
    size_t tb = g_tmp_bytes;
    CK(hipEventRecord(e0, st));
    if constexpr (VALS) CK(rocprim::merge(g_tmp, tb, a, b, out_r, va, vb, vout_r, na, nb, rocprim::less<T>(), st));
    else CK(rocprim::merge(g_tmp, tb, a, b, out_r, na, nb, rocprim::less<T>(), st));
    CK(hipEventRecord(e1, st));
    CK(hipStreamSynchronize(st));
    CK(hipEventElapsedTime(&ms, e0, e1));
    if (r >= 0) tr.push_back(ms * 1000.f);
  }
  *g_badw = 0;
  hipLaunchKernelGGL(count_diff<T>, dim3(2048), dim3(256), 0, st, (const T *)out_d, (const T *)out_r, na + nb, g_badw);
  hipLaunchKernelGGL(count_descents<T>, dim3(2048), dim3(256), 0, st, (const T *)out_d, na + nb, g_badw);
  if constexpr (VALS) hipLaunchKernelGGL(count_diff<V>, dim3(2048), dim3(256), 0, st, (const V *)vout_d, (const V *)vout_r, na + nb, g_badw);
  CK(hipStreamSynchronize(st));
  const Stat d = stat_of(td), r = stat_of(tr);
  const double bytes = 2.0 * (double)(na + nb) * (sizeof(T) + (VALS ? sizeof(V) : 0));
  printf("ROW %s %-22s na=%zu nb=%zu  drhip %9.1f us (%.1f-%.1f)  rocprim %9.1f us (%.1f-%.1f)  drhip/rocprim %.3f  | %.0f GB/s%s\n",
         name_of<T>(), what, na, nb, d.med, d.lo, d.hi, r.med, r.lo, r.hi, d.med / r.med, bytes / d.med / 1e3,
         *g_badw ? "  OUTPUTS DIFFER" : "");
  g_bad += *g_badw != 0;
  fflush(stdout);
  CK(hipEventDestroy(e0));
  CK(hipEventDestroy(e1));
}

// a's values count from 0, b's from b0: every value names its source
template <typename T, typename V>
static void values_row(hipStream_t st, int reps, const char *what, const T *a, const T *b, size_t n, T *out_d, T *out_r, V b0) {
  V *va, *vb, *vo_d, *vo_r;
  CK(hipMalloc(&va, n * sizeof(V)));
  CK(hipMalloc(&vb, n * sizeof(V)));
  CK(hipMalloc(&vo_d, 2 * n * sizeof(V)));
  CK(hipMalloc(&vo_r, 2 * n * sizeof(V)));
  hipLaunchKernelGGL(gen_iota<V>, dim3(4096), dim3(256), 0, st, va, n, V(0));
  hipLaunchKernelGGL(gen_iota<V>, dim3(4096), dim3(256), 0, st, vb, n, b0);
  row<T, V>(st, reps, what, a, n, b, n, out_d, out_r, va, vb, vo_d, vo_r);
  CK(hipFree(va));
  CK(hipFree(vb));
  CK(hipFree(vo_d));
  CK(hipFree(vo_r));
}

template <typename T> static void rows(hipStream_t st, int reps, int log2n, bool all) {
  const size_t n = size_t(1) << log2n, small = std::min(n, size_t(1) << 20);
  T *a, *b, *out_d, *out_r;
  CK(hipMalloc(&a, n * sizeof(T)));
  CK(hipMalloc(&b, n * sizeof(T)));
  CK(hipMalloc(&out_d, 2 * n * sizeof(T)));
  CK(hipMalloc(&out_r, 2 * n * sizeof(T)));
  const char *none = nullptr;
  sort_random(st, out_d, a, n, 11);
  sort_random(st, out_d, b, n, 22);
  row<T, char>(st, reps, "random", a, n, b, n, out_d, out_r, none, none, (char *)nullptr, (char *)nullptr);
  if (all) {
    row<T, char>(st, reps, "random, unbalanced", a, n, b, small, out_d, out_r, none, none, (char *)nullptr, (char *)nullptr);
    values_row<T, uint32_t>(st, reps, "random, u32 values", a, b, n, out_d, out_r, 0x80000000u);
    values_row<T, uint64_t>(st, reps, "random, u64 values", a, b, n, out_d, out_r, uint64_t(1) << 40);
    hipLaunchKernelGGL(gen_ramp<T>, dim3(4096), dim3(256), 0, st, a, n, (T)5, size_t(3));
    hipLaunchKernelGGL(gen_ramp<T>, dim3(4096), dim3(256), 0, st, b, n, (T)(5 + n), size_t(3));
    row<T, char>(st, reps, "a entirely below b", a, n, b, n, out_d, out_r, none, none, (char *)nullptr, (char *)nullptr);
    hipLaunchKernelGGL(gen_ramp<T>, dim3(4096), dim3(256), 0, st, a, n, (T)7, size_t(0));
    hipLaunchKernelGGL(gen_ramp<T>, dim3(4096), dim3(256), 0, st, b, n, (T)7, size_t(0));
    row<T, char>(st, reps, "all keys equal", a, n, b, n, out_d, out_r, none, none, (char *)nullptr, (char *)nullptr);
  }
  CK(hipFree(a));
  CK(hipFree(b));
  CK(hipFree(out_d));
  CK(hipFree(out_r));
}

static void scan_yardstick(hipStream_t st, int reps, int log2n) {
  const size_t n = size_t(2) << log2n;
  uint32_t *in, *out;
  CK(hipMalloc(&in, n * 4));
  CK(hipMalloc(&out, n * 4));
  hipLaunchKernelGGL(gen_random<uint32_t>, dim3(4096), dim3(256), 0, st, in, n, 5ull);
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  std::vector<float> t;
  for (int r = -2; r < reps; r++) {
    float ms;
    CK(hipEventRecord(e0, st));
    CD(drhip_inclusive_scan(0, DRHIP_U32, DRHIP_PLUS, in, out, n, nullptr, nullptr, nullptr, nullptr));
    CK(hipEventRecord(e1, st));
    CK(hipStreamSynchronize(st));
    CK(hipEventElapsedTime(&ms, e0, e1));
    if (r >= 0) t.push_back(ms * 1000.f);
  }
  const Stat s = stat_of(t);
  printf("YARDSTICK drhip_inclusive_scan u32 n=%zu (8 B per element, as a u32 merge of n outputs)  %9.1f us (%.1f-%.1f)  | %.0f GB/s\n",
         n, s.med, s.lo, s.hi, 8.0 * n / s.med / 1e3);
  fflush(stdout);
  CK(hipFree(in));
  CK(hipFree(out));
}

template <typename T, unsigned TILE> static void sweep_one(hipStream_t st, const T *a, const T *b, size_t n, T *out, int cus) {
  using namespace dr_merge;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int per_cu : {2, 4, 8}) {
    std::vector<float> t;
    for (int r = -2; r < 7; r++) {
      float ms;
      CK(hipEventRecord(e0, st));
      CK((mg_enqueue<T, mg_none, TILE, TILE>(st, mg_ptr<T>{a}, n, mg_ptr<T>{b}, n, mg_no_values{}, mg_no_values{}, 0, 2 * n, out,
                                            (mg_none *)nullptr, mg_less{}, (unsigned)(cus * per_cu))));
      CK(hipEventRecord(e1, st));
      CK(hipStreamSynchronize(st));
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= 0) t.push_back(ms * 1000.f);
    }
    const Stat s = stat_of(t);
    printf("SWEEP %s tile=%-5u (%2u items per thread) LDS=%6zu B  %d workgroups per CU  %9.1f us (%.1f-%.1f)\n", name_of<T>(), TILE,
           TILE / 256, (size_t)mg_padded(TILE) * sizeof(T), per_cu, s.med, s.lo, s.hi);
  }
  fflush(stdout);
}
template <typename T> static void sweep(hipStream_t st, int log2n, int cus) {
  const size_t n = size_t(1) << log2n;
  T *a, *b, *out;
  CK(hipMalloc(&a, n * sizeof(T)));
  CK(hipMalloc(&b, n * sizeof(T)));
  CK(hipMalloc(&out, 2 * n * sizeof(T)));
  sort_random(st, out, a, n, 11);
  sort_random(st, out, b, n, 22);
  CK(hipStreamSynchronize(st));
  sweep_one<T, 1024>(st, a, b, n, out, cus);
  sweep_one<T, 2048>(st, a, b, n, out, cus);
  sweep_one<T, 4096>(st, a, b, n, out, cus);
  CK(hipFree(a));
  CK(hipFree(b));
  CK(hipFree(out));
}

int main(int argc, char **argv) {
  bool do_sweep = false;
  std::vector<int> num;
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--sweep")) do_sweep = true;
    else num.push_back(atoi(argv[i]));
  }
  const int reps = num.size() > 0 ? std::max(1, num[0]) : 10;
  const int log2n = num.size() > 1 ? num[1] : 27;
  const size_t n = size_t(1) << log2n;
  shp::init(std::vector<int>{0});
  hipStream_t st = shp::stream(0);
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  printf("merge_bench: 2^%d + 2^%d keys, 2 warm-up + %d timed rounds per row, both implementations once per round, "
         "median (least-greatest) in us, HIP events; tile = %d (4-byte), %d (8-byte)\n",
         log2n, log2n, reps, DRHIP_MERGE_TILE(4), DRHIP_MERGE_TILE(8));
  // rocPRIM's temporary storage: the radix sort of the inputs needs the most
  CK(rocprim::radix_sort_keys(nullptr, g_tmp_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, n, 0, 64, st));
  size_t mb = 0;
  CK(rocprim::merge(nullptr, mb, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr,
                    (uint64_t *)nullptr, (uint64_t *)nullptr, n, n, rocprim::less<uint64_t>(), st));
  g_tmp_bytes = std::max(g_tmp_bytes, mb) + 4096;
  CK(hipMalloc(&g_tmp, g_tmp_bytes));
  CK(hipHostMalloc(&g_badw, 8));
  if (do_sweep) {
    sweep<uint32_t>(st, log2n, prop.multiProcessorCount);
    sweep<uint64_t>(st, log2n, prop.multiProcessorCount);
    shp::finalize();
    return 0;
  }
  rows<uint32_t>(st, reps, log2n, true);
  rows<uint64_t>(st, reps, log2n, false);
  scan_yardstick(st, reps, log2n);
  CK(hipFree(g_tmp));
  shp::finalize();

  // the header layer end to end, 1 and 8 segments (duplicated on the visible devices)
  const size_t ndev = shp::get_numa_devices().size();
  for (std::size_t segs : {std::size_t(1), std::size_t(8)}) {
    shp::init(shp::get_duplicated_devices(shp::get_numa_devices(), segs));
    {
      shp::distributed_vector<uint32_t> a(n), b(n), out(2 * n);
      // sorted across the segments: piece k holds the k-th slice of a ramp with repeats
      for (auto *v : {&a, &b}) {
        std::size_t off = 0;
        for (auto &s : v->segments()) {
          if (s.size())
            hipLaunchKernelGGL(gen_ramp<uint32_t>, dim3(4096), dim3(256), 0, shp::stream(s.rank()), s.data(), s.size(),
                               (uint32_t)(off / 3 + (v == &b ? 1000 : 0)), size_t(3));
          off += (s.size() + 2) / 3 * 3;
        }
      }
      shp::sync_all();
      std::vector<double> t;
      for (int r = -2; r < std::min(reps, 10); r++) {
        auto t0 = std::chrono::steady_clock::now();
        shp::merge(shp::par_unseq, a, b, out);
        auto t1 = std::chrono::steady_clock::now();
        if (r >= 0) t.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
      }
      std::sort(t.begin(), t.end());
      const bool ok = shp::is_sorted(shp::par_unseq, out);
      printf("shp::merge u32 2^%d + 2^%d, %zu segment%s on %zu device%s, end to end: %9.1f us (%.1f-%.1f)%s\n", log2n, log2n, segs,
             segs > 1 ? "s" : "", std::min(segs, ndev), segs > 1 && ndev > 1 ? "s" : "", t[t.size() / 2], t.front(), t.back(),
             ok ? "  sorted" : "  NOT SORTED");
      g_bad += !ok;
    }
    shp::finalize();
  }
  if (ndev < 2) printf("segments on distinct GPUs: unmeasured (one GPU visible)\n");
  return g_bad ? 1 : 0;
}
