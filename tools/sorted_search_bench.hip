// sorted_search_bench.hip -- measurement tool (not product): times
// drhip_lower_bound on ONE device against rocprim::lower_bound (the plain
// per-thread binary search, the yardstick, as rocPRIM's radix sort is for
// tools/sort_bench.hip), in one process on the same buffers.
//   rows: u32 and u64; a sorted haystack of 2^28 (and of 2^16) keys spread
//   evenly over the type's range; m = 2^26 needles that are (a) uniform
//   random, (b) the same needles sorted, (c) all present: drawn from the
//   haystack at random positions.
// Per row: 2 warm-up rounds, then `reps` (default 10) timed rounds; every round
// runs both implementations once (they alternate), HIP events on the segment's
// stream around one call; the median per implementation is printed, in
// microseconds, with the least and the greatest round.  The two outputs are
// compared element by element.  Run the tool at least three times: the bar
// (drhip's median no slower than rocPRIM's by more than the larger run-to-run
// spread) is judged across process runs.
// For information: needles/s x global probes per needle (the levels the
// staging leaves for global memory), next to tools/gather_ceiling's figure;
// shp::lower_bound end to end on 1 and on 8 segments of the visible devices.
// --sweep: the kernel of drhip_lower_bound with S = 1 Ki .. 8 Ki staged
// elements and 2 / 4 / 8 workgroups per CU, 2^28 keys, random needles.
// Build: make -C tools sorted_search_bench.
// Run: tools/sorted_search_bench [reps] [log2n] [log2m] [--sweep]
#include <dr/shp.hpp>

#include <rocprim/device/device_binary_search.hpp>
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
// sorted and evenly spread: x[i] = element first + i of the whole haystack, whose element g holds g in the top
// log2n bits and random bits below
template <typename T> __global__ void gen_sorted(T *x, size_t cnt, size_t first, int log2n, uint64_t seed) {
  const int low = (int)sizeof(T) * 8 - log2n;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < cnt; i += (size_t)gridDim.x * blockDim.x) {
    const uint64_t g = first + i;
    x[i] = (T)((g << low) | (mix(g, seed) & ((1ull << low) - 1)));
  }
}
template <typename T> __global__ void gen_random(T *x, size_t m, uint64_t seed) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x)
    x[i] = (T)mix(i, seed);
}
template <typename T> __global__ void gen_present(T *x, size_t m, const T *hay, size_t n, uint64_t seed) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x)
    x[i] = hay[mix(i, seed) % n];
}
__global__ void count_diff(const uint64_t *a, const uint64_t *b, size_t m, unsigned long long *bad) {
  unsigned long long c = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x) c += a[i] != b[i];
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
static int bits_of(size_t n) {
  int l = 0;
  while (n >> l) l++;
  return l;
}

static int g_bad = 0;

template <typename T> void rows(hipStream_t st, int reps, int log2n, size_t m, void *tmp, size_t tmp_bytes) {
  const size_t n = size_t(1) << log2n;
  T *hay, *nd[3];
  uint64_t *pos_d, *pos_r;
  unsigned long long *bad;
  CK(hipMalloc(&hay, n * sizeof(T)));
  for (auto &p : nd) CK(hipMalloc(&p, m * sizeof(T)));
  CK(hipMalloc(&pos_d, m * 8));
  CK(hipMalloc(&pos_r, m * 8));
  CK(hipHostMalloc(&bad, 8));
  hipLaunchKernelGGL(gen_sorted<T>, dim3(4096), dim3(256), 0, st, hay, n, size_t(0), log2n, 11ull);
  hipLaunchKernelGGL(gen_random<T>, dim3(4096), dim3(256), 0, st, nd[0], m, 22ull);
  size_t sb = tmp_bytes;
  CK(rocprim::radix_sort_keys(tmp, sb, nd[0], nd[1], m, 0, sizeof(T) * 8, st));
  hipLaunchKernelGGL(gen_present<T>, dim3(4096), dim3(256), 0, st, nd[2], m, (const T *)hay, n, 33ull);
  CK(hipStreamSynchronize(st));
  const char *sets[3] = {"random ", "sorted ", "present"};
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const int S = DRHIP_SORTED_SEARCH_STAGE(sizeof(T));
  const int probes = m >= (size_t)S ? std::max(0, bits_of(n) - bits_of(S) + 1) : bits_of(n);
  for (int s = 0; s < 3; s++) {
    std::vector<float> td, tr;
    for (int r = -2; r < reps; r++) {
      float ms;
      CK(hipEventRecord(e0, st));
      CD(drhip_lower_bound(0, dtype_of<T>(), hay, n, nd[s], m, pos_d));
      CK(hipEventRecord(e1, st));
      CK(hipStreamSynchronize(st));
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= 0) td.push_back(ms * 1000.f);
      size_t tb = tmp_bytes;
      CK(hipEventRecord(e0, st));
      CK(rocprim::lower_bound(tmp, tb, (const T *)hay, (const T *)nd[s], pos_r, n, m, rocprim::less<T>(), st));
      CK(hipEventRecord(e1, st));
      CK(hipStreamSynchronize(st));
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= 0) tr.push_back(ms * 1000.f);
    }
    *bad = 0;
    hipLaunchKernelGGL(count_diff, dim3(2048), dim3(256), 0, st, (const uint64_t *)pos_d, (const uint64_t *)pos_r, m, bad);
    CK(hipStreamSynchronize(st));
    const Stat d = stat_of(td), r = stat_of(tr);
    printf("ROW %s n=2^%d m=2^%d %s  drhip_lower_bound %9.1f us (%.1f-%.1f)  rocprim::lower_bound %9.1f us (%.1f-%.1f)  "
           "drhip/rocprim %.3f  | %d global probes per needle: %.1f G probes/s%s\n",
           name_of<T>(), log2n, bits_of(m) - 1, sets[s], d.med, d.lo, d.hi, r.med, r.lo, r.hi, d.med / r.med, probes,
           (double)m * probes / d.med / 1e3, *bad ? "  OUTPUTS DIFFER" : "");
    g_bad += *bad != 0;
  }
  fflush(stdout);
  CK(hipFree(hay));
  for (auto &p : nd) CK(hipFree(p));
  CK(hipFree(pos_d));
  CK(hipFree(pos_r));
  CK(hipHostFree(bad));
}

template <typename T, int S> void sweep_one(hipStream_t st, const T *hay, size_t n, const T *nd, size_t m, uint64_t *pos, int cus) {
  using namespace dr_bsearch;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int per_cu : {2, 4, 8}) {
    std::vector<float> t;
    for (int r = -2; r < 7; r++) {
      float ms;
      CK(hipEventRecord(e0, st));
      CK((bs_enqueue<T, BS_POS, S, false>(st, bs_one<T, bs_ptr<T>>{bs_ptr<T>{hay}}, n, bs_span<T>{nd}, m, bs_lower<bs_less>{},
                                          pos, (unsigned)(cus * per_cu))));
      CK(hipEventRecord(e1, st));
      CK(hipStreamSynchronize(st));
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= 0) t.push_back(ms * 1000.f);
    }
    const Stat s = stat_of(t);
    printf("SWEEP %s S=%-5d LDS=%6zu B  %d workgroups per CU  %9.1f us (%.1f-%.1f)\n", name_of<T>(), S, (size_t)S * sizeof(T),
           per_cu, s.med, s.lo, s.hi);
  }
  fflush(stdout);
}
template <typename T> void sweep(hipStream_t st, int log2n, size_t m, int cus) {
  const size_t n = size_t(1) << log2n;
  T *hay, *nd;
  uint64_t *pos;
  CK(hipMalloc(&hay, n * sizeof(T)));
  CK(hipMalloc(&nd, m * sizeof(T)));
  CK(hipMalloc(&pos, m * 8));
  hipLaunchKernelGGL(gen_sorted<T>, dim3(4096), dim3(256), 0, st, hay, n, size_t(0), log2n, 11ull);
  hipLaunchKernelGGL(gen_random<T>, dim3(4096), dim3(256), 0, st, nd, m, 22ull);
  CK(hipStreamSynchronize(st));
  sweep_one<T, 1024>(st, hay, n, nd, m, pos, cus);
  sweep_one<T, 2048>(st, hay, n, nd, m, pos, cus);
  sweep_one<T, 4096>(st, hay, n, nd, m, pos, cus);
  sweep_one<T, 8192>(st, hay, n, nd, m, pos, cus);
  CK(hipFree(hay));
  CK(hipFree(nd));
  CK(hipFree(pos));
}

int main(int argc, char **argv) {
  bool do_sweep = false;
  std::vector<int> num;
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--sweep")) do_sweep = true;
    else num.push_back(atoi(argv[i]));
  }
  const int reps = num.size() > 0 ? std::max(1, num[0]) : 10;
  const int log2n = num.size() > 1 ? num[1] : 28;
  const int log2m = num.size() > 2 ? num[2] : 26;
  const size_t m = size_t(1) << log2m;
  shp::init(std::vector<int>{0});
  hipStream_t st = shp::stream(0);
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  printf("sorted_search_bench: m = 2^%d needles, 2 warm-up + %d timed rounds per row, both implementations once per round, "
         "median (least-greatest) in us, HIP events; S = %d (4-byte), %d (8-byte)\n",
         log2m, reps, DRHIP_SORTED_SEARCH_STAGE(4), DRHIP_SORTED_SEARCH_STAGE(8));
  if (do_sweep) {
    sweep<uint32_t>(st, log2n, m, prop.multiProcessorCount);
    sweep<uint64_t>(st, log2n, m, prop.multiProcessorCount);
    shp::finalize();
    return 0;
  }
  // rocPRIM's temporary storage: the radix sort of the needles needs the most
  size_t tmp_bytes = 0;
  CK(rocprim::radix_sort_keys(nullptr, tmp_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, m, 0, 64, st));
  tmp_bytes += 4096;
  void *tmp;
  CK(hipMalloc(&tmp, tmp_bytes));
  for (int l : {log2n, 16}) {
    rows<uint32_t>(st, reps, l, m, tmp, tmp_bytes);
    rows<uint64_t>(st, reps, l, m, tmp, tmp_bytes);
  }
  printf("tools/gather_ceiling (profiles/r03_gather_ceiling.txt): 51-56 G random 4-byte gathers/s\n");
  CK(hipFree(tmp));
  shp::finalize();

  // the header layer end to end, 1 and 8 segments (duplicated on the visible devices)
  const size_t n = size_t(1) << log2n;
  const size_t ndev = shp::get_numa_devices().size();
  for (std::size_t segs : {std::size_t(1), std::size_t(8)}) {
    shp::init(shp::get_duplicated_devices(shp::get_numa_devices(), segs));
    {
      shp::distributed_vector<uint32_t> hay(n), nd(m);
      shp::distributed_vector<uint64_t> pos(m);
      std::size_t off = 0;
      for (auto &s : hay.segments()) {
        hipLaunchKernelGGL(gen_sorted<uint32_t>, dim3(4096), dim3(256), 0, shp::stream(s.rank()), s.data(), s.size(), off, log2n,
                           11ull);
        off += s.size();
      }
      shp::sync_all();
      for (auto &s : nd.segments())
        hipLaunchKernelGGL(gen_random<uint32_t>, dim3(4096), dim3(256), 0, shp::stream(s.rank()), s.data(), s.size(),
                           22ull + s.rank());
      shp::sync_all();
      std::vector<double> t;
      for (int r = -2; r < std::min(reps, 10); r++) {
        auto t0 = std::chrono::steady_clock::now();
        shp::lower_bound(shp::par_unseq, hay, nd, pos);
        auto t1 = std::chrono::steady_clock::now();
        if (r >= 0) t.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
      }
      std::sort(t.begin(), t.end());
      // check: every position p has hay[p - 1] < needle <= hay[p], through the scalar form on a few needles
      bool ok = true;
      std::vector<uint32_t> some(64);
      std::vector<uint64_t> got(64);
      shp::copy(nd.begin(), nd.begin() + 64, some.data());
      shp::copy(pos.begin(), pos.begin() + 64, got.data());
      for (int i = 0; i < 64; i++)
        ok = ok && (std::size_t)(shp::lower_bound(shp::par_unseq, hay, some[i]) - hay.begin()) == got[i];
      printf("shp::lower_bound u32 n=2^%d m=2^%d, %zu segment%s on %zu device%s, end to end: %9.1f us (%.1f-%.1f)%s\n", log2n,
             log2m, segs, segs > 1 ? "s" : "", std::min(segs, ndev), segs > 1 && ndev > 1 ? "s" : "", t[t.size() / 2],
             t.front(), t.back(), ok ? "  ok" : "  WRONG");
      g_bad += !ok;
    }
    shp::finalize();
  }
  if (ndev < 2) printf("segments on distinct GPUs: unmeasured (one GPU visible)\n");
  return g_bad ? 1 : 0;
}
