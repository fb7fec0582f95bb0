// decaf377::Engine::vartime_multiscalar_mul_short and msm_short_resident (include/decaf377_amd.hpp) on the GPU: sums of 1, 65
// and 700 terms over uint64_t, unsigned __int128 and 16-byte records against vartime_multiscalar_mul on the same values
// zero-extended to Fr and against the fold of the mirror's own `*` (mul) and `+` (add); the resident form on buffers of
// hipMalloc against the host form; a refused scalar length.  Built and run by tests/test_msm_short_gpu.py (-m gpu).
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

  for (const size_t n : {size_t(1), size_t(65), size_t(700)}) {
    std::vector<Fq> seeds(n);
    std::vector<uint64_t> k64(n);
    std::vector<unsigned __int128> k128(n);
    std::vector<std::array<uint8_t, 16>> rec(n);
    std::vector<Fr> f64(n), f128(n);
    for (size_t i = 0; i < n; ++i) {
      seeds[i].b[0] = (uint8_t)(i + 1); seeds[i].b[1] = (uint8_t)((i + 1) >> 8); seeds[i].b[2] = (uint8_t)n;
      k64[i] = i == 0 ? ~0ull : rng();
      k128[i] = i == 0 ? ~(unsigned __int128)0 : ((unsigned __int128)rng() << 64) | rng();
      std::memcpy(rec[i].data(), &k128[i], 16);
      std::memcpy(f64[i].b.data(), &k64[i], 8);                  // zero-extended to 32 bytes
      std::memcpy(f128[i].b.data(), &k128[i], 16);
    }
    const std::vector<Element> pts = e.encode_to_curve_element(seeds);

    // the fold of the mirror's own operations
    const std::vector<Element> prod = e.mul(pts, f128);
    std::vector<Element> acc(1, prod[0]);
    for (size_t i = 1; i < n; ++i) acc = e.add(acc, std::vector<Element>(1, prod[i]));
    const Encoding fold = e.vartime_compress(acc)[0];

    Encoding enc64, enc128, encrec;
    const Element s64 = e.vartime_multiscalar_mul_short(k64, pts, &enc64);
    const Element s128 = e.vartime_multiscalar_mul_short(k128, pts, &enc128);
    const Element srec = e.vartime_multiscalar_mul_short(rec, pts, &encrec);
    const Encoding want64 = e.vartime_compress({e.vartime_multiscalar_mul(f64, pts)})[0];
    const Encoding want128 = e.vartime_compress({e.vartime_multiscalar_mul(f128, pts)})[0];
    CHECK(enc64 == want64);
    CHECK(enc128 == want128 && encrec == want128 && enc128 == fold);
    CHECK(e.vartime_compress({s64})[0] == enc64 && e.vartime_compress({s128})[0] == enc128 && e.vartime_compress({srec})[0] == enc128);

    DevBuf<Element> dpts(pts);
    DevBuf<uint64_t> dk64(k64);
    DevBuf<unsigned __int128> dk128(k128);
    DevBuf<Encoding> enc(1);
    DevBuf<Element> el(1);
    e.msm_short_resident(0, s, dpts.p, dk64.p, 8, n, enc.p, el.p);
    CHECK(enc.host(s)[0] == enc64 && e.vartime_compress(el.host(s))[0] == enc64);
    e.msm_short_resident(0, s, dpts.p, dk128.p, 16, n, enc.p);
    CHECK(enc.host(s)[0] == enc128);
    const std::vector<Encoding> encs = e.vartime_compress(pts);
    DevBuf<Encoding> dencs(encs);
    DevBuf<uint8_t> st(n);
    e.msm_short_resident(0, s, dencs.p, dk128.p, 16, n, enc.p, el.p, st.p);
    CHECK(enc.host(s)[0] == enc128);
    for (const uint8_t b : st.host(s)) CHECK(b == 0);

    bool threw = false;
    try { e.msm_short_resident(0, s, dpts.p, dk64.p, 12, n, enc.p); }
    catch (const DeviceError&) { threw = true; }
    CHECK(threw);
  }
  bool threw = false;
  try { e.vartime_multiscalar_mul_short(std::vector<uint64_t>(2), std::vector<Element>(3, Engine::identity())); }
  catch (const std::invalid_argument&) { threw = true; }
  CHECK(threw);
  HIP_OK(hipStreamDestroy(s));
  std::printf("CPP_MSM_SHORT_OK\n");
  return 0;
}
