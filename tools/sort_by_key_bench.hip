// sort_by_key_bench.hip -- measurement tool (not product): times the by-key
// sort on ONE device against the only by-key route there was before it,
// shp::sort of a distributed_vector<struct{key, value}> with a key-comparing
// lambda (the general merge tier, dr/shp/merge_sort.hpp), plus drhip_sort
// keys-only at 2^28 u32 as the unchanged yardstick.
//   * drhip_sort_pairs, 2^28 pairs: u32 keys + u32 values, u32 + u64
//   * drhip_sort_pairs, 2^27 pairs: u64 keys + u64 values
// Every figure: 3 warm-up calls, then `reps` (default 20) timed calls, HIP
// events on the segment's stream around the device work of one call (the
// input is restored outside the events); median and range.  Every result is
// checked on the device: keys ascending, and equal keys with ascending
// values (the values are the input positions, so that is stability).
// Build: make -C tools sort_by_key_bench.   Run: tools/sort_by_key_bench [reps] [log2n]
#include <dr/shp.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
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

template <typename K, typename V> struct Rec {
  K key;
  V val;
};

__device__ inline uint64_t mix(uint64_t i, uint64_t seed) {
  uint64_t h = (i + 1) * 0x9E3779B97F4A7C15ull ^ seed;
  h ^= h >> 31;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 29;
  return h;
}
template <typename K, typename V> __global__ void gen_pairs(K *k, V *v, size_t n, uint64_t seed) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    k[i] = (K)mix(i, seed);
    if (v) v[i] = (V)i;
  }
}
template <typename K, typename V> __global__ void gen_recs(Rec<K, V> *r, size_t n, uint64_t seed) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    r[i] = Rec<K, V>{(K)mix(i, seed), (V)i};
}
// bad += positions out of key order, or equal keys out of value order
template <typename K, typename V>
__global__ void check_pairs(const K *k, const V *v, size_t n, unsigned long long *bad) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x + 1; i < n; i += (size_t)gridDim.x * blockDim.x)
    if (k[i - 1] > k[i] || (v && k[i - 1] == k[i] && v[i - 1] > v[i])) atomicAdd(bad, 1ull);
}
template <typename K, typename V> __global__ void check_recs(const Rec<K, V> *r, size_t n, unsigned long long *bad) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x + 1; i < n; i += (size_t)gridDim.x * blockDim.x)
    if (r[i - 1].key > r[i].key || (r[i - 1].key == r[i].key && r[i - 1].val > r[i].val)) atomicAdd(bad, 1ull);
}

struct Stat {
  double med, lo, hi;
};
static Stat stat_of(std::vector<float> t) {
  std::sort(t.begin(), t.end());
  return {t[t.size() / 2], t.front(), t.back()};
}
constexpr int kWarm = 3;

// restore() puts the input back (outside the events), call() enqueues / runs one sort
template <typename Restore, typename Call> static Stat time_calls(hipStream_t st, int reps, Restore restore, Call call) {
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  std::vector<float> t;
  for (int r = -kWarm; r < reps; r++) {
    restore();
    CK(hipEventRecord(e0, st));
    call();
    CK(hipEventRecord(e1, st));
    CK(hipStreamSynchronize(st));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    if (r >= 0) t.push_back(ms);
  }
  CK(hipEventDestroy(e0));
  CK(hipEventDestroy(e1));
  return stat_of(t);
}

static unsigned long long read_bad(unsigned long long *d_bad, hipStream_t st) {
  unsigned long long h = 0;
  CK(hipMemcpyAsync(&h, d_bad, 8, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  return h;
}

template <typename K> constexpr int key_code() {
  return sizeof(K) == 4 ? DRHIP_U32 : DRHIP_U64;
}

// the pairs sort and the struct-and-lambda route at the same n; returns the ratio
template <typename K, typename V> static void run_case(int log2n, int reps, hipStream_t st, unsigned long long *d_bad) {
  const size_t n = size_t(1) << log2n;
  const char *name = sizeof(K) == 4 ? (sizeof(V) == 4 ? "u32+u32" : "u32+u64") : "u64+u64";
  Stat pairs, recs;
  unsigned long long bad_p, bad_r;
  {
    K *k, *ks;
    V *v, *vs;
    CK(hipMalloc(&k, n * sizeof(K)));
    CK(hipMalloc(&ks, n * sizeof(K)));
    CK(hipMalloc(&v, n * sizeof(V)));
    CK(hipMalloc(&vs, n * sizeof(V)));
    hipLaunchKernelGGL((gen_pairs<K, V>), dim3(4096), dim3(256), 0, st, ks, vs, n, 12345ull);
    size_t wsb = 0;
    CD(drhip_sort_pairs_workspace(0, key_code<K>(), sizeof(V), n, &wsb));
    void *ws;
    CK(hipMalloc(&ws, wsb));
    pairs = time_calls(
        st, reps,
        [&] {
          CK(hipMemcpyAsync(k, ks, n * sizeof(K), hipMemcpyDeviceToDevice, st));
          CK(hipMemcpyAsync(v, vs, n * sizeof(V), hipMemcpyDeviceToDevice, st));
        },
        [&] { CD(drhip_sort_pairs(0, key_code<K>(), k, v, sizeof(V), n, ws, wsb)); });
    CK(hipMemsetAsync(d_bad, 0, 8, st));
    hipLaunchKernelGGL((check_pairs<K, V>), dim3(4096), dim3(256), 0, st, k, v, n, d_bad);
    bad_p = read_bad(d_bad, st);
    for (void *p : {(void *)k, (void *)ks, (void *)v, (void *)vs, ws}) CK(hipFree(p));
  }
  {
    using R = Rec<K, V>;
    shp::distributed_vector<R> dv(n);
    R *seg = dv.segments()[0].data();
    auto by_key = [](const R &a, const R &b) { return a.key < b.key; };
    recs = time_calls(
        st, reps, [&] { hipLaunchKernelGGL((gen_recs<K, V>), dim3(4096), dim3(256), 0, st, seg, n, 12345ull); },
        [&] { shp::sort(shp::par_unseq, dv, by_key); });
    CK(hipMemsetAsync(d_bad, 0, 8, st));
    hipLaunchKernelGGL((check_recs<K, V>), dim3(4096), dim3(256), 0, st, seg, n, d_bad);
    bad_r = read_bad(d_bad, st);
  }
  printf("%s n=2^%d  drhip_sort_pairs           %8.3f ms (%.3f-%.3f)  %6.2f Gpairs/s  out_of_order=%llu\n", name, log2n,
         pairs.med, pairs.lo, pairs.hi, n / pairs.med / 1e6, bad_p);
  printf("%s n=2^%d  shp::sort(struct, lambda)  %8.3f ms (%.3f-%.3f)  %6.2f Gpairs/s  out_of_order=%llu  (%zu-byte struct)\n",
         name, log2n, recs.med, recs.lo, recs.hi, n / recs.med / 1e6, bad_r, sizeof(Rec<K, V>));
  printf("%s n=2^%d  ratio struct / pairs = %.2fx\n", name, log2n, recs.med / pairs.med);
  fflush(stdout);
}

int main(int argc, char **argv) {
  const int reps = argc > 1 ? std::max(1, atoi(argv[1])) : 20;
  const int log2n = argc > 2 ? atoi(argv[2]) : 28;
  shp::init(std::vector<int>{0});
  hipStream_t st = shp::stream(0);
  unsigned long long *d_bad;
  CK(hipMalloc(&d_bad, 8));
  printf("sort_by_key_bench: %d warm-up + %d timed calls per figure, median (min-max), HIP events\n", kWarm, reps);
  {
    // keys only, the yardstick that must not have moved
    const size_t n = size_t(1) << log2n;
    uint32_t *k, *ks;
    CK(hipMalloc(&k, n * 4));
    CK(hipMalloc(&ks, n * 4));
    hipLaunchKernelGGL((gen_pairs<uint32_t, uint32_t>), dim3(4096), dim3(256), 0, st, ks, (uint32_t *)nullptr, n,
                       12345ull);
    size_t wsb = 0;
    CD(drhip_sort_workspace(0, DRHIP_U32, n, &wsb));
    void *ws;
    CK(hipMalloc(&ws, wsb));
    const Stat s = time_calls(
        st, reps, [&] { CK(hipMemcpyAsync(k, ks, n * 4, hipMemcpyDeviceToDevice, st)); },
        [&] { CD(drhip_sort(0, DRHIP_U32, k, n, ws, wsb)); });
    CK(hipMemsetAsync(d_bad, 0, 8, st));
    hipLaunchKernelGGL((check_pairs<uint32_t, uint32_t>), dim3(4096), dim3(256), 0, st, k, (const uint32_t *)nullptr, n,
                       d_bad);
    printf("u32 keys only n=2^%d  drhip_sort        %8.3f ms (%.3f-%.3f)  %6.2f Gkeys/s  out_of_order=%llu\n", log2n,
           s.med, s.lo, s.hi, n / s.med / 1e6, read_bad(d_bad, st));
    fflush(stdout);
    for (void *p : {(void *)k, (void *)ks, ws}) CK(hipFree(p));
  }
  run_case<uint32_t, uint32_t>(log2n, reps, st, d_bad);
  run_case<uint32_t, uint64_t>(log2n, reps, st, d_bad);
  run_case<uint64_t, uint64_t>(log2n - 1, reps, st, d_bad);
  CK(hipFree(d_bad));
  shp::finalize();
  return 0;
}
