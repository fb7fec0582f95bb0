// decaf377::Engine::vartime_multiscalar_mul_batch_buckets and msm_buckets_resident (include/decaf377_amd.hpp) on the GPU: sums
// of 5, 40 and 129 terms, with the library's window width and a forced one, against the fold of the mirror's own `*` (mul)
// and `+` (add); the resident form on buffers of hipMalloc against the host form; a sum of identities.  Built and run by
// tests/test_bucket_sums_gpu.py (-m gpu).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "decaf377_amd.hpp"

using namespace decaf377;

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)
#define HIP_OK(e) CHECK((e) == hipSuccess)

template <class T>
struct DevBuf {                                                // a hipMalloc'ed copy of a host vector
  T* p = nullptr;
  size_t n;
  explicit DevBuf(size_t count) : n(count) { HIP_OK(hipMalloc(reinterpret_cast<void**>(&p), (count ? count : 1) * sizeof(T))); }
  explicit DevBuf(const std::vector<T>& h) : DevBuf(h.size()) { HIP_OK(hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice)); }
  ~DevBuf() { (void)hipFree(p); }
  std::vector<T> host(hipStream_t s) const {
    std::vector<T> h(n);
    HIP_OK(hipStreamSynchronize(s));
    HIP_OK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    return h;
  }
};

int main() {
  std::mt19937_64 rng(377);
  Engine e({0}, 18, true);
  HIP_OK(hipSetDevice(0));
  hipStream_t s;
  HIP_OK(hipStreamCreate(&s));
  const Element identity = Engine::identity();

  for (const size_t m : {size_t(5), size_t(40), size_t(129)}) {
    const size_t n = 6, terms = n * m;
    std::vector<Fq> seeds(terms);
    std::vector<Fr> k(terms);
    for (size_t i = 0; i < terms; ++i) {
      seeds[i].b[0] = (uint8_t)(i + 1); seeds[i].b[1] = (uint8_t)((i + 1) >> 8); seeds[i].b[2] = (uint8_t)m;
      for (int b = 0; b < 31; ++b) k[i].b[b] = (uint8_t)rng();
    }
    std::vector<Element> pts = e.encode_to_curve_element(seeds);
    for (size_t j = 0; j < m; ++j) pts[(n - 1) * m + j] = identity;   // the last sum: the identity

    std::vector<Element> prod = e.mul(pts, k);
    std::vector<Element> acc(n), col(n);
    for (size_t i = 0; i < n; ++i) acc[i] = prod[i * m];
    for (size_t j = 1; j < m; ++j) {
      for (size_t i = 0; i < n; ++i) col[i] = prod[i * m + j];
      acc = e.add(acc, col);
    }
    const std::vector<Encoding> want = e.vartime_compress(acc);

    for (const int window_bits : {0, 12}) {
      std::vector<Encoding> encs;
      const std::vector<Element> sums = e.vartime_multiscalar_mul_batch_buckets(m, k, pts, &encs, window_bits);
      CHECK(sums.size() == n && encs.size() == n);
      CHECK(encs == want);
      CHECK(e.vartime_compress(sums) == encs);
      CHECK(encs[n - 1] == Encoding{});

      DevBuf<Element> dpts(pts);
      DevBuf<Fr> dk(k);
      DevBuf<Encoding> enc(n);
      DevBuf<Element> el(n);
      e.msm_buckets_resident(0, s, dpts.p, dk.p, m, n, enc.p, el.p, window_bits);
      CHECK(enc.host(s) == encs);
      CHECK(e.vartime_compress(el.host(s)) == encs);
    }
  }
  bool threw = false;
  try { e.vartime_multiscalar_mul_batch_buckets(1, std::vector<Fr>(2), std::vector<Element>(2, identity), nullptr, 17); }
  catch (const DeviceError&) { threw = true; }
  CHECK(threw);
  HIP_OK(hipStreamDestroy(s));
  std::printf("CPP_BUCKET_SUMS_OK\n");
  return 0;
}
