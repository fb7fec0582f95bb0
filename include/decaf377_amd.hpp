// decaf377_amd.hpp -- C++ host-side mirror of the reference crate's hot-path API over the C ABI.
//
// Same names and error behaviour as penumbra-zone/decaf377 (v0.10.1), batch-shaped:
//   decaf377::Encoding            Encoding(pub [u8; 32])             src/ark_curve/encoding.rs:14-15
//   decaf377::Element             opaque X, Y, Z, T Montgomery limbs  src/min_curve/element.rs:31-38
//   decaf377::Fq / Fr             32-byte little-endian field elements src/fields/fq.rs, fr.rs
//   decaf377::EncodingError       InvalidEncoding / InvalidSliceLength src/error.rs:1-5
// Header-only; link with -ldecaf377_amd.  All computation happens on the GPU.
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "decaf377_amd.h"

namespace decaf377 {

enum class EncodingError { InvalidEncoding, InvalidSliceLength };

struct DeviceError : std::runtime_error {
  explicit DeviceError(int code) : std::runtime_error(std::string("decaf377_amd: ") + d377_last_error()), code(code) {}
  int code;
  // D377_ERR_STARVED: workgroups found no free lane set for 10 s; the call wrote nothing usable (Context health / reset_scratch)
  bool starved() const { return code == D377_ERR_STARVED; }
};

// Result<T, EncodingError>
template <class T>
struct Result {
  bool ok;
  T value;
  EncodingError err;
  const T& unwrap() const {
    if (!ok) throw std::runtime_error("called unwrap() on Err(InvalidEncoding)");
    return value;
  }
  bool is_err() const { return !ok; }
};

struct Bytes32 {
  std::array<uint8_t, 32> b{};
  bool operator==(const Bytes32& o) const { return b == o.b; }
  bool operator!=(const Bytes32& o) const { return !(*this == o); }
};

namespace detail {
// little-endian comparison of a 32-byte string against a modulus given as 4 u64 limbs
inline bool lt_modulus(const std::array<uint8_t, 32>& v, const uint64_t (&m)[4]) {
  for (int i = 3; i >= 0; --i) {
    uint64_t w = 0;
    for (int j = 7; j >= 0; --j) w = (w << 8) | v[8 * i + j];
    if (w != m[i]) return w < m[i];
  }
  return false;
}
}  // namespace detail

struct Fq : Bytes32 {
  // src/fields/fq.rs:29-34
  static constexpr uint64_t MODULUS_LIMBS[4] = {725501752471715841ULL, 6461107452199829505ULL,
                                                6968279316240510977ULL, 1345280370688173398ULL};
  /// Fq::from_le_bytes_mod_order: the bytes are carried as-is; the engine reduces them mod q.
  static Fq from_le_bytes_mod_order(const uint8_t* bytes32) { Fq f; std::memcpy(f.b.data(), bytes32, 32); return f; }
  /// Fq::from_bytes_checked (src/fields/fq.rs:108-115)
  static Result<Fq> from_bytes_checked(const std::array<uint8_t, 32>& bytes) {
    Fq f; f.b = bytes;
    return {detail::lt_modulus(bytes, MODULUS_LIMBS), f, EncodingError::InvalidEncoding};
  }
  static Fq from_u64(uint64_t x) { Fq f; for (int i = 0; i < 8; ++i) f.b[i] = (uint8_t)(x >> (8 * i)); return f; }
  std::array<uint8_t, 32> to_bytes() const { return b; }
};

struct Fr : Bytes32 {
  // src/fields/fr.rs:29-34
  static constexpr uint64_t MODULUS_LIMBS[4] = {13356249993388743167ULL, 5950279507993463550ULL,
                                                10965441865914903552ULL, 336320092672043349ULL};
  static Fr from_le_bytes_mod_order(const uint8_t* bytes32) { Fr f; std::memcpy(f.b.data(), bytes32, 32); return f; }
  static Result<Fr> from_bytes_checked(const std::array<uint8_t, 32>& bytes) {
    Fr f; f.b = bytes;
    return {detail::lt_modulus(bytes, MODULUS_LIMBS), f, EncodingError::InvalidEncoding};
  }
  static Fr from_u64(uint64_t x) { Fr f; for (int i = 0; i < 8; ++i) f.b[i] = (uint8_t)(x >> (8 * i)); return f; }
};

struct Encoding : Bytes32 {
  Encoding() = default;
  explicit Encoding(const std::array<uint8_t, 32>& a) { b = a; }
  /// TryFrom<&[u8]> (src/ark_curve/encoding.rs:131-143): wrong length -> InvalidSliceLength
  static Result<Encoding> try_from(const uint8_t* data, size_t len) {
    Encoding e;
    if (len != 32) return {false, e, EncodingError::InvalidSliceLength};
    std::memcpy(e.b.data(), data, 32);
    return {true, e, EncodingError::InvalidEncoding};
  }
};

struct Element {
  std::array<uint64_t, 16> xyzt{};   // X, Y, Z, T; 4 Montgomery limbs each (R = 2^256)
};

static_assert(sizeof(Encoding) == 32 && sizeof(Fq) == 32 && sizeof(Fr) == 32 && sizeof(Element) == 128,
              "records must be packed");

/// Which backend's root sqrt_ratio_zeta returns: the arkworks one (Sarkar tables, src/ark_curve/invsqrt.rs:75-166)
/// or the min_curve one (Tonelli-Shanks seeded with 11^m, src/min_curve/invsqrt.rs:11-95).  Same flags.
enum class SqrtRoot : int { Ark = D377_SQRT_ROOT_ARK, MinCurve = D377_SQRT_ROOT_MIN_CURVE };

class Engine;

/// Fixed-base combs for caller-chosen points (d377_fixed_bases_create): ark-ec's FixedBase window tables over any Element
/// (src/ark_curve/element.rs:22-38), one comb per base on every device of the Engine.  Move-only; made by
/// Engine::fixed_bases.  The Engine must outlive it in the usual order, and if it does not, ~Engine releases the tables
/// and leaves this object empty: every later call throws, and its destructor does nothing.
class FixedBases {
 public:
  FixedBases(FixedBases&& o) noexcept;
  FixedBases& operator=(FixedBases&& o) noexcept;
  FixedBases(const FixedBases&) = delete;
  FixedBases& operator=(const FixedBases&) = delete;
  ~FixedBases() { reset(); }

  size_t size() const { return m_; }                        // m, the number of bases
  /// n sums, sum i = scalars[i m] * B_0 + ... + scalars[i m + m - 1] * B_{m-1} (scalars term-major), as Encodings;
  /// `elements`, if given, receives the sums as Elements (some extended representative), which the same pass computes.
  std::vector<Encoding> vartime_multiscalar_mul(const std::vector<Fr>& scalars, std::vector<Element>* elements = nullptr) {
    if (!h_) throw std::logic_error("decaf377_amd: FixedBases used after it was destroyed or its Engine was");
    if (scalars.size() % m_) throw std::invalid_argument("length mismatch: scalars must be n x m");
    std::vector<Encoding> enc(scalars.size() / m_);
    if (elements) elements->assign(enc.size(), Element{});
    const int rc = d377_batch_fixed_msm(ctx(), h_, reinterpret_cast<const uint8_t*>(scalars.data()), enc.size(),
                                        reinterpret_cast<uint8_t*>(enc.data()),
                                        elements ? reinterpret_cast<uint64_t*>(elements->data()) : nullptr);
    if (rc != D377_OK) throw DeviceError(rc);
    return enc;
  }
  /// The same sums with every sum cut into segments of consecutive bases, one GPU lane per segment, where that fills the chip
  /// (d377_batch_fixed_long_msm; long_plan shows the cut): few sums over many bases.  Any FixedBases, short or long.
  std::vector<Encoding> msm_long(const std::vector<Fr>& scalars, std::vector<Element>* elements = nullptr) {
    if (!h_) throw std::logic_error("decaf377_amd: FixedBases used after it was destroyed or its Engine was");
    if (scalars.size() % m_) throw std::invalid_argument("length mismatch: scalars must be n x m");
    std::vector<Encoding> enc(scalars.size() / m_);
    if (elements) elements->assign(enc.size(), Element{});
    const int rc = d377_batch_fixed_long_msm(ctx(), h_, reinterpret_cast<const uint8_t*>(scalars.data()), enc.size(),
                                             reinterpret_cast<uint8_t*>(enc.data()),
                                             elements ? reinterpret_cast<uint64_t*>(elements->data()) : nullptr);
    if (rc != D377_OK) throw DeviceError(rc);
    return enc;
  }
  /// {segments per sum, bases per segment} of msm_long for the slice of n sums that device `dev` of the Engine gets
  /// (d377_fixed_long_msm_plan).
  std::pair<size_t, size_t> long_plan(size_t n, int dev = 0) const {
    if (!h_) throw std::logic_error("decaf377_amd: FixedBases used after it was destroyed or its Engine was");
    uint64_t g = 0, b = 0;
    const int rc = d377_fixed_long_msm_plan(ctx(), h_, n, dev, &g, &b);
    if (rc != D377_OK) throw DeviceError(rc);
    return {(size_t)g, (size_t)b};
  }
  /// n sums of t terms that name their bases: sum i = sum over j < t of scalars[i t + j] * B_{base_index[i t + j]} (both
  /// term-major, n x t each).  An index is 0 .. size() - 1, or -1 for an absent term (which costs as much as a present
  /// one); anything else makes the library refuse the call (DeviceError, nothing computed).
  std::vector<Encoding> msm_indexed(const std::vector<int>& base_index, const std::vector<Fr>& scalars, size_t t,
                                    std::vector<Element>* elements = nullptr) {
    if (!h_) throw std::logic_error("decaf377_amd: FixedBases used after it was destroyed or its Engine was");
    if (t == 0 || scalars.size() % t || base_index.size() != scalars.size())
      throw std::invalid_argument("length mismatch: base_index and scalars must be n x t");
    std::vector<Encoding> enc(scalars.size() / t);
    if (elements) elements->assign(enc.size(), Element{});
    const int rc = d377_batch_fixed_msm_indexed(ctx(), h_, base_index.data(), reinterpret_cast<const uint8_t*>(scalars.data()), t,
                                                enc.size(), reinterpret_cast<uint8_t*>(enc.data()),
                                                elements ? reinterpret_cast<uint64_t*>(elements->data()) : nullptr);
    if (rc != D377_OK) throw DeviceError(rc);
    return enc;
  }
  /// n mixed sums: sum i = sum over j < t of fixed_scalars[i t + j] * B_{base_index[i t + j]} + sum over p < v of
  /// var_scalars[i v + p] * points[i v + p] (d377_batch_msm_mixed; all term-major, 1 <= t <= 64, 1 <= v <= 8).  The check of a
  /// signature R' = s B - c A is t = v = 1.  Index -1 is an absent term; any index outside -1 .. size() - 1 makes the library
  /// refuse the call (DeviceError, nothing computed).
  std::vector<Encoding> msm_mixed(const std::vector<int>& base_index, const std::vector<Fr>& fixed_scalars, size_t t,
                                  const std::vector<Element>& points, const std::vector<Fr>& var_scalars, size_t v,
                                  std::vector<Element>* elements = nullptr) {
    if (!h_) throw std::logic_error("decaf377_amd: FixedBases used after it was destroyed or its Engine was");
    if (t == 0 || v == 0 || fixed_scalars.size() % t || base_index.size() != fixed_scalars.size() || points.size() % v ||
        var_scalars.size() != points.size() || points.size() / v != fixed_scalars.size() / t)
      throw std::invalid_argument("length mismatch: base_index and fixed_scalars must be n x t, points and var_scalars n x v");
    std::vector<Encoding> enc(fixed_scalars.size() / t);
    if (elements) elements->assign(enc.size(), Element{});
    const int rc = d377_batch_msm_mixed(ctx(), h_, base_index.data(), reinterpret_cast<const uint8_t*>(fixed_scalars.data()), t,
                                        reinterpret_cast<const uint64_t*>(points.data()),
                                        reinterpret_cast<const uint8_t*>(var_scalars.data()), v, enc.size(),
                                        reinterpret_cast<uint8_t*>(enc.data()),
                                        elements ? reinterpret_cast<uint64_t*>(elements->data()) : nullptr);
    if (rc != D377_OK) throw DeviceError(rc);
    return enc;
  }
  /// The same sums over Encodings (d377_batch_msm_mixed_encoded): status[i v + p] = 1 marks an invalid Encoding, whose term
  /// alone is left out of its sum.
  std::vector<Encoding> msm_mixed(const std::vector<int>& base_index, const std::vector<Fr>& fixed_scalars, size_t t,
                                  const std::vector<Encoding>& points, const std::vector<Fr>& var_scalars, size_t v,
                                  std::vector<uint8_t>* status, std::vector<Element>* elements = nullptr) {
    if (!h_) throw std::logic_error("decaf377_amd: FixedBases used after it was destroyed or its Engine was");
    if (t == 0 || v == 0 || fixed_scalars.size() % t || base_index.size() != fixed_scalars.size() || points.size() % v ||
        var_scalars.size() != points.size() || points.size() / v != fixed_scalars.size() / t)
      throw std::invalid_argument("length mismatch: base_index and fixed_scalars must be n x t, points and var_scalars n x v");
    std::vector<Encoding> enc(fixed_scalars.size() / t);
    std::vector<uint8_t> st(points.size(), 0);
    if (elements) elements->assign(enc.size(), Element{});
    const int rc = d377_batch_msm_mixed_encoded(ctx(), h_, base_index.data(), reinterpret_cast<const uint8_t*>(fixed_scalars.data()), t,
                                                reinterpret_cast<const uint8_t*>(points.data()),
                                                reinterpret_cast<const uint8_t*>(var_scalars.data()), v, enc.size(),
                                                reinterpret_cast<uint8_t*>(enc.data()),
                                                elements ? reinterpret_cast<uint64_t*>(elements->data()) : nullptr, st.data());
    if (rc != D377_OK) throw DeviceError(rc);
    if (status) status->swap(st);
    return enc;
  }
  /// The resident forms (d377_batch_*_resident): every pointer is a DEVICE pointer on device `dev` of the Engine (records
  /// 16-byte aligned), the call enqueues on `stream` (a hipStream_t) and returns without synchronising; n sums.  `elements_out`
  /// and `verdict` may be null.  The indexed and mixed forms do not refuse a bad index: it contributes nothing and the
  /// verdict record (two u64 on the device: the count of refused indices, the first position or UINT64_MAX) counts it.
  void msm_resident(int dev, void* stream, const Fr* scalars, size_t n, Encoding* enc_out, Element* elements_out = nullptr) {
    live();
    check(d377_batch_fixed_msm_resident(ctx(), dev, stream, h_, reinterpret_cast<const uint8_t*>(scalars), n,
                                        reinterpret_cast<uint8_t*>(enc_out), reinterpret_cast<uint64_t*>(elements_out)));
  }
  void msm_long_resident(int dev, void* stream, const Fr* scalars, size_t n, Encoding* enc_out, Element* elements_out = nullptr) {
    live();
    check(d377_batch_fixed_long_msm_resident(ctx(), dev, stream, h_, reinterpret_cast<const uint8_t*>(scalars), n,
                                             reinterpret_cast<uint8_t*>(enc_out), reinterpret_cast<uint64_t*>(elements_out)));
  }
  void msm_indexed_resident(int dev, void* stream, const int* base_index, const Fr* scalars, size_t t, size_t n, Encoding* enc_out,
                            Element* elements_out = nullptr, uint64_t* verdict = nullptr) {
    live();
    check(d377_batch_fixed_msm_indexed_resident(ctx(), dev, stream, h_, base_index, reinterpret_cast<const uint8_t*>(scalars), t, n,
                                                reinterpret_cast<uint8_t*>(enc_out), reinterpret_cast<uint64_t*>(elements_out), verdict));
  }
  void msm_mixed_resident(int dev, void* stream, const int* base_index, const Fr* fixed_scalars, size_t t, const Element* points,
                          const Fr* var_scalars, size_t v, size_t n, Encoding* enc_out, Element* elements_out = nullptr,
                          uint64_t* verdict = nullptr) {
    live();
    check(d377_batch_msm_mixed_resident(ctx(), dev, stream, h_, base_index, reinterpret_cast<const uint8_t*>(fixed_scalars), t,
                                        reinterpret_cast<const uint64_t*>(points), reinterpret_cast<const uint8_t*>(var_scalars), v, n,
                                        reinterpret_cast<uint8_t*>(enc_out), reinterpret_cast<uint64_t*>(elements_out), verdict));
  }
  /// ... over Encodings: status (n x v device bytes) marks the invalid ones
  void msm_mixed_resident(int dev, void* stream, const int* base_index, const Fr* fixed_scalars, size_t t, const Encoding* points,
                          const Fr* var_scalars, size_t v, size_t n, Encoding* enc_out, uint8_t* status, Element* elements_out = nullptr,
                          uint64_t* verdict = nullptr) {
    live();
    check(d377_batch_msm_mixed_encoded_resident(ctx(), dev, stream, h_, base_index, reinterpret_cast<const uint8_t*>(fixed_scalars), t,
                                                reinterpret_cast<const uint8_t*>(points), reinterpret_cast<const uint8_t*>(var_scalars),
                                                v, n, reinterpret_cast<uint8_t*>(enc_out), reinterpret_cast<uint64_t*>(elements_out),
                                                status, verdict));
  }
  /// The index verdict alone over `count` device ints (d377_check_base_index_resident).
  void check_base_index_resident(int dev, void* stream, const int* base_index, size_t count, uint64_t* verdict) {
    live();
    check(d377_check_base_index_resident(ctx(), dev, stream, h_, base_index, count, verdict));
  }
  /// table bytes per device
  uint64_t table_bytes() const {
    uint64_t b = 0;
    if (h_) d377_fixed_bases_info(ctx(), h_, nullptr, nullptr, &b);
    return b;
  }
  explicit operator bool() const { return h_ != 0; }

 private:
  friend class Engine;
  FixedBases(Engine* e, int64_t h, size_t m) : eng_(e), h_(h), m_(m) {}
  void live() const { if (!h_) throw std::logic_error("decaf377_amd: FixedBases used after it was destroyed or its Engine was"); }
  static void check(int rc) { if (rc != D377_OK) throw DeviceError(rc); }
  void reset();
  d377_ctx* ctx() const;
  Engine* eng_ = nullptr;
  int64_t h_ = 0;                                           // the context's handle; 0 = empty
  size_t m_ = 0;
};

/// Owns one d377_ctx (device tables, streams, scratch).  Calls on one Engine are serialised inside the library.
class Engine {
 public:
  explicit Engine(const std::vector<int>& device_ids = {0}) {
    int rc = d377_ctx_create(device_ids.data(), (int)device_ids.size(), &ctx_);
    if (rc != D377_OK) throw DeviceError(rc);
  }
  /// With the fixed-base comb's options (d377_ctx_create_ex): comb_bits 0 (default: 23), 18, 21 or 23; comb_lazy: the table
  /// is built by the first GENERATOR * Fr batch -- Element::GENERATOR is a constant in the crate (src/min_curve/element.rs:61-81).
  Engine(const std::vector<int>& device_ids, int comb_bits, bool comb_lazy) {
    d377_ctx_opts o{sizeof(d377_ctx_opts), comb_bits, comb_lazy ? 1 : 0};
    int rc = d377_ctx_create_ex(device_ids.data(), (int)device_ids.size(), &o, &ctx_);
    if (rc != D377_OK) throw DeviceError(rc);
  }
  ~Engine() {
    {
      std::lock_guard<std::mutex> lock(fixed_mu_);
      for (FixedBases* fb : fixed_) { fb->h_ = 0; fb->eng_ = nullptr; }   // d377_ctx_destroy releases their tables
      fixed_.clear();
    }
    d377_ctx_destroy(ctx_);
  }
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;

  /// Registers 1 .. 64 fixed bases (D377_FIXED_BASES_MAX) and builds their combs: comb_bits 8, 12, 16 or 18 (0.53 / 5.5 /
  /// 67 / 235 MB per base and device; 32 / 21 / 16 / 14 mixed additions per base and sum).
  FixedBases fixed_bases(const std::vector<Element>& bases, int comb_bits = 16) {
    int64_t h = 0;
    check(d377_fixed_bases_create(ctx_, u64(bases), bases.size(), comb_bits, &h));
    FixedBases fb(this, h, bases.size());
    std::lock_guard<std::mutex> lock(fixed_mu_);
    fixed_.push_back(&fb);
    return fb;                                            // (moved out: the move constructor re-registers the new address)
  }
  /// Registers 1 .. 4096 fixed bases (D377_FIXED_BASES_LONG_MAX, d377_fixed_bases_create_long): 4096 bases are 2.2 GB at
  /// comb_bits 8 and 22.5 GB at 12, per device.  vartime_multiscalar_mul on more than 64 bases is msm_long.
  FixedBases fixed_bases_long(const std::vector<Element>& bases, int comb_bits = 12) {
    int64_t h = 0;
    check(d377_fixed_bases_create_long(ctx_, u64(bases), bases.size(), comb_bits, &h));
    FixedBases fb(this, h, bases.size());
    std::lock_guard<std::mutex> lock(fixed_mu_);
    fixed_.push_back(&fb);
    return fb;
  }

  /// Encoding::vartime_decompress, one Result per input (src/ark_curve/encoding.rs:32-83)
  std::vector<Result<Element>> vartime_decompress(const std::vector<Encoding>& encs) {
    std::vector<Element> out(encs.size());
    std::vector<uint8_t> st(encs.size());
    check(d377_batch_decompress(ctx_, u8(encs), encs.size(), reinterpret_cast<uint64_t*>(out.data()), st.data()));
    return results(out, st);
  }
  /// Element::vartime_compress (src/ark_curve/encoding.rs:116-128)
  std::vector<Encoding> vartime_compress(const std::vector<Element>& els) {
    std::vector<Encoding> out(els.size());
    check(d377_batch_compress(ctx_, reinterpret_cast<const uint64_t*>(els.data()), els.size(), u8m(out)));
    return out;
  }
  /// Element::encode_to_curve, compressed (src/ark_curve/elligator.rs:74-76)
  std::vector<Encoding> encode_to_curve(const std::vector<Fq>& rs) {
    std::vector<Encoding> out(rs.size());
    check(d377_batch_encode_to_curve(ctx_, u8(rs), rs.size(), u8m(out)));
    return out;
  }
  /// Element::hash_to_curve, compressed (src/ark_curve/elligator.rs:67-71)
  std::vector<Encoding> hash_to_curve(const std::vector<Fq>& r1, const std::vector<Fq>& r2) {
    if (r1.size() != r2.size()) throw std::invalid_argument("length mismatch");
    std::vector<Encoding> out(r1.size());
    check(d377_batch_hash_to_curve(ctx_, u8(r1), u8(r2), r1.size(), u8m(out)));
    return out;
  }
  /// Element::GENERATOR * k, compressed
  std::vector<Encoding> mul_generator(const std::vector<Fr>& ks) {
    std::vector<Encoding> out(ks.size());
    check(d377_batch_scalar_mul_base(ctx_, u8(ks), ks.size(), u8m(out)));
    return out;
  }
  /// decompress(P)? * k, compressed (src/min_curve/ops.rs:89-95)
  std::vector<Result<Encoding>> scalar_mul(const std::vector<Encoding>& ps, const std::vector<Fr>& ks) {
    if (ps.size() != ks.size()) throw std::invalid_argument("length mismatch");
    std::vector<Encoding> out(ps.size());
    std::vector<uint8_t> st(ps.size());
    check(d377_batch_scalar_mul_var(ctx_, u8(ps), u8(ks), ps.size(), u8m(out), st.data()));
    return results(out, st);
  }
  /// Element * Fr, Elements in and out (`impl Mul<Fr> for Element`, src/min_curve/ops.rs:89-95)
  std::vector<Element> mul(const std::vector<Element>& ps, const std::vector<Fr>& ks) {
    if (ps.size() != ks.size()) throw std::invalid_argument("length mismatch");
    std::vector<Element> out(ps.size());
    check(d377_batch_scalar_mul_var_element(ctx_, u64(ps), u8(ks), ps.size(), reinterpret_cast<uint64_t*>(out.data())));
    return out;
  }
  /// Element::GENERATOR * k as Elements
  std::vector<Element> mul_generator_element(const std::vector<Fr>& ks) {
    std::vector<Element> out(ks.size());
    check(d377_batch_scalar_mul_base_element(ctx_, u8(ks), ks.size(), reinterpret_cast<uint64_t*>(out.data())));
    return out;
  }
  /// Element::encode_to_curve / hash_to_curve as Elements (src/min_curve/element.rs:235-244)
  std::vector<Element> encode_to_curve_element(const std::vector<Fq>& rs) {
    std::vector<Element> out(rs.size());
    check(d377_batch_encode_to_curve_element(ctx_, u8(rs), rs.size(), reinterpret_cast<uint64_t*>(out.data())));
    return out;
  }
  std::vector<Element> hash_to_curve_element(const std::vector<Fq>& r1, const std::vector<Fq>& r2) {
    if (r1.size() != r2.size()) throw std::invalid_argument("length mismatch");
    std::vector<Element> out(r1.size());
    check(d377_batch_hash_to_curve_element(ctx_, u8(r1), u8(r2), r1.size(), reinterpret_cast<uint64_t*>(out.data())));
    return out;
  }
  /// Element::vartime_compress_to_field (src/min_curve/element.rs:163-181): 4 Montgomery limbs per element
  std::vector<std::array<uint64_t, 4>> vartime_compress_to_field(const std::vector<Element>& els) {
    std::vector<std::array<uint64_t, 4>> out(els.size());
    check(d377_batch_compress_to_field(ctx_, u64(els), els.size(), reinterpret_cast<uint64_t*>(out.data())));
    return out;
  }
  /// Fr + - * (src/fields/fr/u64/wrapper.rs:88-108); square / neg take b empty; inverse: ok = false for zero (:80-86)
  std::vector<Result<Fr>> fr_op(int op, const std::vector<Fr>& a, const std::vector<Fr>& b = {}) {
    const bool binary = op <= D377_FQ_MUL;
    if (binary && a.size() != b.size()) throw std::invalid_argument("length mismatch");
    std::vector<Fr> out(a.size());
    std::vector<uint8_t> st(a.size());
    check(d377_batch_fr_op(ctx_, op, u8(a), binary ? u8(b) : nullptr, a.size(), u8m(out), st.data()));
    return results(out, st);
  }
  std::vector<Fr> fr_add(const std::vector<Fr>& a, const std::vector<Fr>& b) { return values(fr_op(D377_FQ_ADD, a, b)); }
  std::vector<Fr> fr_sub(const std::vector<Fr>& a, const std::vector<Fr>& b) { return values(fr_op(D377_FQ_SUB, a, b)); }
  std::vector<Fr> fr_mul(const std::vector<Fr>& a, const std::vector<Fr>& b) { return values(fr_op(D377_FQ_MUL, a, b)); }
  /// Fr::from_le_bytes_mod_order on n strings of len = 48 or 64 bytes (src/fields/fr.rs:82-94)
  std::vector<Fr> fr_from_wide_bytes(const std::vector<uint8_t>& bytes, size_t len) {
    if (len == 0 || bytes.size() % len) throw std::invalid_argument("length mismatch");
    std::vector<Fr> out(bytes.size() / len);
    check(d377_batch_fr_from_wide_bytes(ctx_, bytes.data(), len, out.size(), u8m(out)));
    return out;
  }
  /// Fq::sqrt_ratio_zeta (src/ark_curve/invsqrt.rs:75-166; SqrtRoot::MinCurve: src/min_curve/invsqrt.rs:73-95)
  std::vector<std::pair<bool, Fq>> sqrt_ratio_zeta(const std::vector<Fq>& num, const std::vector<Fq>& den,
                                                   SqrtRoot which = SqrtRoot::Ark) {
    if (num.size() != den.size()) throw std::invalid_argument("length mismatch");
    std::vector<Fq> root(num.size());
    std::vector<uint8_t> ws(num.size());
    check(d377_batch_sqrt_ratio_zeta_ex(ctx_, (int)which, u8(num), u8(den), num.size(), u8m(root), ws.data()));
    std::vector<std::pair<bool, Fq>> r(num.size());
    for (size_t i = 0; i < r.size(); ++i) r[i] = {ws[i] != 0, root[i]};
    return r;
  }
  /// Element + Element / double / == (src/min_curve/element.rs:291-340)
  std::vector<Element> add(const std::vector<Element>& p, const std::vector<Element>& q) {
    if (p.size() != q.size()) throw std::invalid_argument("length mismatch");
    std::vector<Element> out(p.size());
    check(d377_batch_add(ctx_, u64(p), u64(q), p.size(), reinterpret_cast<uint64_t*>(out.data())));
    return out;
  }
  /// Element - Element (src/min_curve/ops.rs:43-87)
  std::vector<Element> sub(const std::vector<Element>& p, const std::vector<Element>& q) {
    if (p.size() != q.size()) throw std::invalid_argument("length mismatch");
    std::vector<Element> out(p.size());
    check(d377_batch_sub(ctx_, u64(p), u64(q), p.size(), reinterpret_cast<uint64_t*>(out.data())));
    return out;
  }
  std::vector<Element> double_(const std::vector<Element>& p) {
    std::vector<Element> out(p.size());
    check(d377_batch_double(ctx_, u64(p), p.size(), reinterpret_cast<uint64_t*>(out.data())));
    return out;
  }
  std::vector<bool> eq(const std::vector<Element>& p, const std::vector<Element>& q) {
    if (p.size() != q.size()) throw std::invalid_argument("length mismatch");
    std::vector<uint8_t> e(p.size());
    check(d377_batch_eq(ctx_, u64(p), u64(q), p.size(), e.data()));
    return std::vector<bool>(e.begin(), e.end());
  }
  /// -Element and Element::is_identity (src/min_curve/element.rs:324-332, 113-117)
  std::vector<Element> neg(const std::vector<Element>& p) {
    std::vector<Element> out(p.size());
    check(d377_batch_neg(ctx_, u64(p), p.size(), reinterpret_cast<uint64_t*>(out.data())));
    return out;
  }
  std::vector<bool> is_identity(const std::vector<Element>& p) {
    std::vector<uint8_t> e(p.size());
    check(d377_batch_is_identity(ctx_, u64(p), p.size(), e.data()));
    return std::vector<bool>(e.begin(), e.end());
  }
  /// Element::vartime_multiscalar_mul(scalars, points) (src/ark_curve/element/projective.rs:99-117)
  Element vartime_multiscalar_mul(const std::vector<Fr>& scalars, const std::vector<Element>& points) {
    if (scalars.size() != points.size()) throw std::invalid_argument("length mismatch");
    Element out;
    Encoding enc;
    check(d377_msm(ctx_, u64(points), u8(scalars), points.size(), enc.b.data(), out.xyzt.data()));
    return out;
  }
  /// The same over Encodings: invalid ones are reported (Err) and left out of the sum.
  std::pair<Element, std::vector<Result<Encoding>>> vartime_multiscalar_mul_encoded(const std::vector<Fr>& scalars,
                                                                                   const std::vector<Encoding>& points) {
    if (scalars.size() != points.size()) throw std::invalid_argument("length mismatch");
    Element out;
    Encoding enc;
    std::vector<uint8_t> st(points.size() ? points.size() : 1);
    check(d377_msm_encoded(ctx_, u8(points), u8(scalars), points.size(), enc.b.data(), out.xyzt.data(), st.data()));
    st.resize(points.size());
    return {out, results(points, st)};
  }
  /// The same over scalars that are SHORT by their type -- uint64_t or unsigned __int128: the weights of a batch verification,
  /// amounts (d377_msm_short, decaf377_amd_short_msm.h).  The Element (and Encoding) is that of vartime_multiscalar_mul on the
  /// same values, from 5 or 9 windows of digits instead of 16.  Scalars are passed as they lie in memory (little-endian hosts).
  Element vartime_multiscalar_mul_short(const std::vector<uint64_t>& scalars, const std::vector<Element>& points, Encoding* encoding = nullptr) {
    return msm_short_host(scalars.data(), 8, scalars.size(), points, encoding);
  }
  Element vartime_multiscalar_mul_short(const std::vector<unsigned __int128>& scalars, const std::vector<Element>& points,
                                        Encoding* encoding = nullptr) {
    return msm_short_host(scalars.data(), 16, scalars.size(), points, encoding);
  }
  /// ... 16-byte little-endian records, for callers that hold their u128 values as bytes
  Element vartime_multiscalar_mul_short(const std::vector<std::array<uint8_t, 16>>& scalars, const std::vector<Element>& points,
                                        Encoding* encoding = nullptr) {
    return msm_short_host(scalars.data(), 16, scalars.size(), points, encoding);
  }
  /// ... on DEVICE pointers of device `dev` of the Engine: `scalars` holds n records of scalar_bytes (8 or 16) bytes and is
  /// aligned to that, the other records 16-byte aligned; enqueues on `stream` and returns.  d377_msm_dev's workspace rules: one
  /// eager call of a shape before it is captured into a graph.
  void msm_short_resident(int dev, void* stream, const Element* points, const void* scalars, int scalar_bytes, size_t n, Encoding* enc_out,
                          Element* element_out = nullptr) {
    check(d377_msm_short_dev(ctx_, dev, stream, reinterpret_cast<const uint64_t*>(points), static_cast<const uint8_t*>(scalars), scalar_bytes, n,
                             reinterpret_cast<uint8_t*>(enc_out), reinterpret_cast<uint64_t*>(element_out)));
  }
  void msm_short_resident(int dev, void* stream, const Encoding* points, const void* scalars, int scalar_bytes, size_t n, Encoding* enc_out,
                          Element* element_out, uint8_t* status) {
    check(d377_msm_short_encoded_dev(ctx_, dev, stream, reinterpret_cast<const uint8_t*>(points), static_cast<const uint8_t*>(scalars), scalar_bytes,
                                     n, reinterpret_cast<uint8_t*>(enc_out), reinterpret_cast<uint64_t*>(element_out), status));
  }
  /// MANY small sums at once: sum i = scalars[i m ..][..m] . points[i m ..][..m], m terms each (1 .. 8) -- the shape of the
  /// crate's own multiscalar test, a 3-term sum per case (tests/operations.rs:44-60).  The sums come back as Elements, as
  /// the crate's function returns them; `encodings`, if given, receives their Encodings, which the same pass computes.
  std::vector<Element> vartime_multiscalar_mul_batch(size_t m, const std::vector<Fr>& scalars, const std::vector<Element>& points,
                                                     std::vector<Encoding>* encodings = nullptr) {
    if (scalars.size() != points.size() || m == 0 || points.size() % m) throw std::invalid_argument("length mismatch");
    std::vector<Element> out(points.size() / m);
    std::vector<Encoding> enc(out.size());
    check(d377_batch_msm_small(ctx_, u64(points), u8(scalars), m, out.size(), u8m(enc), reinterpret_cast<uint64_t*>(out.data())));
    if (encodings) *encodings = std::move(enc);
    return out;
  }
  /// The same over Encodings: an invalid one is reported (Err, per term) and left out of its sum.
  std::pair<std::vector<Element>, std::vector<Result<Encoding>>> vartime_multiscalar_mul_batch_encoded(
      size_t m, const std::vector<Fr>& scalars, const std::vector<Encoding>& points, std::vector<Encoding>* encodings = nullptr) {
    if (scalars.size() != points.size() || m == 0 || points.size() % m) throw std::invalid_argument("length mismatch");
    std::vector<Element> out(points.size() / m);
    std::vector<Encoding> enc(out.size());
    std::vector<uint8_t> st(points.size() ? points.size() : 1);
    check(d377_batch_msm_small_encoded(ctx_, u8(points), u8(scalars), m, out.size(), u8m(enc), reinterpret_cast<uint64_t*>(out.data()), st.data()));
    st.resize(points.size());
    if (encodings) *encodings = std::move(enc);
    return {out, results(points, st)};
  }
  /// MANY sums of medium length at once: the sums of vartime_multiscalar_mul_batch with 1 <= m <= 4096 terms each
  /// (d377_batch_msm_long: every sum cut into chains of at most 8 terms, the partial sums folded on the device).  Host
  /// vectors only; for ONE long sum use vartime_multiscalar_mul.
  std::vector<Element> vartime_multiscalar_mul_batch_long(size_t m, const std::vector<Fr>& scalars, const std::vector<Element>& points,
                                                          std::vector<Encoding>* encodings = nullptr) {
    if (scalars.size() != points.size() || m == 0 || points.size() % m) throw std::invalid_argument("length mismatch");
    std::vector<Element> out(points.size() / m);
    std::vector<Encoding> enc(out.size());
    check(d377_batch_msm_long(ctx_, u64(points), u8(scalars), m, out.size(), u8m(enc), reinterpret_cast<uint64_t*>(out.data())));
    if (encodings) *encodings = std::move(enc);
    return out;
  }
  /// The same over Encodings: an invalid one is reported (Err, per term) and left out of its sum.
  std::pair<std::vector<Element>, std::vector<Result<Encoding>>> vartime_multiscalar_mul_batch_long_encoded(
      size_t m, const std::vector<Fr>& scalars, const std::vector<Encoding>& points, std::vector<Encoding>* encodings = nullptr) {
    if (scalars.size() != points.size() || m == 0 || points.size() % m) throw std::invalid_argument("length mismatch");
    std::vector<Element> out(points.size() / m);
    std::vector<Encoding> enc(out.size());
    std::vector<uint8_t> st(points.size() ? points.size() : 1);
    check(d377_batch_msm_long_encoded(ctx_, u8(points), u8(scalars), m, out.size(), u8m(enc), reinterpret_cast<uint64_t*>(out.data()), st.data()));
    st.resize(points.size());
    if (encodings) *encodings = std::move(enc);
    return {out, results(points, st)};
  }
  /// Long sums whose terms name their points in a shared pool (d377_batch_long_msm_indexed): sum i = sum over j < m of
  /// scalars[i m + j] * pool[point_index[i m + j]], -1 an absent term.  Any other index outside the pool throws and nothing
  /// is computed.
  std::vector<Element> vartime_multiscalar_mul_batch_long_indexed(size_t m, const std::vector<Element>& pool, const std::vector<int>& point_index,
                                                                  const std::vector<Fr>& scalars, std::vector<Encoding>* encodings = nullptr) {
    if (scalars.size() != point_index.size() || m == 0 || point_index.size() % m) throw std::invalid_argument("length mismatch");
    std::vector<Element> out(point_index.size() / m);
    std::vector<Encoding> enc(out.size());
    check(d377_batch_long_msm_indexed(ctx_, u64(pool), pool.size(), point_index.data(), u8(scalars), m, out.size(), u8m(enc),
                                      reinterpret_cast<uint64_t*>(out.data())));
    if (encodings) *encodings = std::move(enc);
    return out;
  }
  /// The resident forms of the long sums (decaf377_amd_long_sums.h): every pointer is a DEVICE pointer on device `dev` of the
  /// Engine (records 16-byte aligned), the call enqueues on `stream` and returns.  elements_out and verdict may be null; an
  /// index outside the pool contributes nothing and is counted in `verdict` (two u64: the count, the first position).
  void msm_long_resident(int dev, void* stream, const Element* points, const Fr* scalars, size_t m, size_t n, Encoding* enc_out,
                         Element* elements_out = nullptr) {
    check(d377_batch_long_msm_resident(ctx_, dev, stream, reinterpret_cast<const uint64_t*>(points), reinterpret_cast<const uint8_t*>(scalars), m, n,
                                       reinterpret_cast<uint8_t*>(enc_out), reinterpret_cast<uint64_t*>(elements_out)));
  }
  void msm_long_resident(int dev, void* stream, const Encoding* points, const Fr* scalars, size_t m, size_t n, Encoding* enc_out,
                         Element* elements_out, uint8_t* status) {
    check(d377_batch_long_msm_encoded_resident(ctx_, dev, stream, reinterpret_cast<const uint8_t*>(points), reinterpret_cast<const uint8_t*>(scalars),
                                               m, n, reinterpret_cast<uint8_t*>(enc_out), reinterpret_cast<uint64_t*>(elements_out), status));
  }
  void msm_long_indexed_resident(int dev, void* stream, const Element* pool, size_t pool_count, const int* point_index, const Fr* scalars,
                                 size_t m, size_t n, Encoding* enc_out, Element* elements_out = nullptr, uint64_t* verdict = nullptr) {
    check(d377_batch_long_msm_indexed_resident(ctx_, dev, stream, reinterpret_cast<const uint64_t*>(pool), pool_count, point_index,
                                               reinterpret_cast<const uint8_t*>(scalars), m, n, reinterpret_cast<uint8_t*>(enc_out),
                                               reinterpret_cast<uint64_t*>(elements_out), verdict));
  }
  /// MANY sums of up to 2^20 terms each by the bucket method (d377_batch_bucket_msm, decaf377_amd_bucket_sums.h): the sums of a
  /// pass share one run of vartime_multiscalar_mul's sort / span / bucket pipeline.  window_bits: 0 = the library's rule,
  /// 4 .. 16 forces the window width (a developer and test knob).
  std::vector<Element> vartime_multiscalar_mul_batch_buckets(size_t m, const std::vector<Fr>& scalars, const std::vector<Element>& points,
                                                             std::vector<Encoding>* encodings = nullptr, int window_bits = 0) {
    if (scalars.size() != points.size() || m == 0 || points.size() % m) throw std::invalid_argument("length mismatch");
    std::vector<Element> out(points.size() / m);
    std::vector<Encoding> enc(out.size());
    check(d377_batch_bucket_msm(ctx_, u64(points), u8(scalars), m, out.size(), window_bits, u8m(enc), reinterpret_cast<uint64_t*>(out.data())));
    if (encodings) *encodings = std::move(enc);
    return out;
  }
  /// ... on DEVICE pointers of device `dev` of the Engine (records 16-byte aligned): enqueues on `stream` and returns.  One eager
  /// call of a shape must come before it is captured into a graph (the MSM workspace cannot grow inside a capture).
  void msm_buckets_resident(int dev, void* stream, const Element* points, const Fr* scalars, size_t m, size_t n, Encoding* enc_out,
                            Element* elements_out = nullptr, int window_bits = 0) {
    check(d377_batch_bucket_msm_resident(ctx_, dev, stream, reinterpret_cast<const uint64_t*>(points), reinterpret_cast<const uint8_t*>(scalars), m, n,
                                         window_bits, reinterpret_cast<uint8_t*>(enc_out), reinterpret_cast<uint64_t*>(elements_out)));
  }
  void msm_buckets_resident(int dev, void* stream, const Encoding* points, const Fr* scalars, size_t m, size_t n, Encoding* enc_out,
                            Element* elements_out, uint8_t* status, int window_bits = 0) {
    check(d377_batch_bucket_msm_encoded_resident(ctx_, dev, stream, reinterpret_cast<const uint8_t*>(points), reinterpret_cast<const uint8_t*>(scalars),
                                                 m, n, window_bits, reinterpret_cast<uint8_t*>(enc_out), reinterpret_cast<uint64_t*>(elements_out),
                                                 status));
  }
  /// MANY sums of ANY length each, 0 .. 2^20 terms per sum (d377_batch_ragged_msm, decaf377_amd_ragged_sums.h): sum i is the terms
  /// offsets[i] .. offsets[i + 1] - 1; offsets holds n + 1 values, starts at 0, never decreases and ends at points.size().  An
  /// empty sum is the identity.  No short-sum route: see the header's "which call where".  window_bits as above.
  std::vector<Element> vartime_multiscalar_mul_batch_ragged(const std::vector<uint64_t>& offsets, const std::vector<Fr>& scalars,
                                                            const std::vector<Element>& points, std::vector<Encoding>* encodings = nullptr,
                                                            int window_bits = 0) {
    if (scalars.size() != points.size() || offsets.empty() || offsets.back() != points.size()) throw std::invalid_argument("length mismatch");
    std::vector<Element> out(offsets.size() - 1);
    std::vector<Encoding> enc(out.size());
    check(d377_batch_ragged_msm(ctx_, u64(points), u8(scalars), offsets.data(), out.size(), window_bits, u8m(enc),
                                reinterpret_cast<uint64_t*>(out.data())));
    if (encodings) *encodings = std::move(enc);
    return out;
  }
  /// ... on DEVICE pointers of device `dev` of the Engine (records 16-byte aligned): enqueues on `stream` and returns.  `offsets`
  /// (n + 1 values, HOST memory) is read before the call returns; the kernels read `offsets_dev`, the same values on the device
  /// (8-byte aligned).  Nothing can check that the two agree: if they do not, the sums are wrong (memory stays safe).  One eager
  /// call of a shape must come before it is captured into a graph.
  void msm_ragged_resident(int dev, void* stream, const Element* points, const Fr* scalars, const uint64_t* offsets, const uint64_t* offsets_dev,
                           size_t n, Encoding* enc_out, Element* elements_out = nullptr, int window_bits = 0) {
    check(d377_batch_ragged_msm_resident(ctx_, dev, stream, reinterpret_cast<const uint64_t*>(points), reinterpret_cast<const uint8_t*>(scalars),
                                         offsets, offsets_dev, n, window_bits, reinterpret_cast<uint8_t*>(enc_out),
                                         reinterpret_cast<uint64_t*>(elements_out)));
  }
  void msm_ragged_resident(int dev, void* stream, const Encoding* points, const Fr* scalars, const uint64_t* offsets, const uint64_t* offsets_dev,
                           size_t n, Encoding* enc_out, Element* elements_out, uint8_t* status, int window_bits = 0) {
    check(d377_batch_ragged_msm_encoded_resident(ctx_, dev, stream, reinterpret_cast<const uint8_t*>(points), reinterpret_cast<const uint8_t*>(scalars),
                                                 offsets, offsets_dev, n, window_bits, reinterpret_cast<uint8_t*>(enc_out),
                                                 reinterpret_cast<uint64_t*>(elements_out), status));
  }
  /// The same sums by Straus chains (d377_batch_segmented_msm, decaf377_amd_segmented_sums.h): every sum cut into chains of at
  /// most 8 terms, as vartime_multiscalar_mul_batch_long cuts sums of one length -- the call for MANY SHORT sums of unequal
  /// length.  The Encodings are vartime_multiscalar_mul_batch_ragged's; the Elements are some representative of the same sums.
  std::vector<Element> vartime_multiscalar_mul_batch_segmented(const std::vector<uint64_t>& offsets, const std::vector<Fr>& scalars,
                                                               const std::vector<Element>& points, std::vector<Encoding>* encodings = nullptr) {
    if (scalars.size() != points.size() || offsets.empty() || offsets.back() != points.size()) throw std::invalid_argument("length mismatch");
    std::vector<Element> out(offsets.size() - 1);
    std::vector<Encoding> enc(out.size());
    check(d377_batch_segmented_msm(ctx_, u64(points), u8(scalars), offsets.data(), out.size(), u8m(enc), reinterpret_cast<uint64_t*>(out.data())));
    if (encodings) *encodings = std::move(enc);
    return out;
  }
  /// ... on DEVICE pointers: msm_ragged_resident's contract without window_bits.  The kernels read `offsets_dev` alone.
  void msm_segmented_resident(int dev, void* stream, const Element* points, const Fr* scalars, const uint64_t* offsets,
                              const uint64_t* offsets_dev, size_t n, Encoding* enc_out, Element* elements_out = nullptr) {
    check(d377_batch_segmented_msm_resident(ctx_, dev, stream, reinterpret_cast<const uint64_t*>(points), reinterpret_cast<const uint8_t*>(scalars),
                                            offsets, offsets_dev, n, reinterpret_cast<uint8_t*>(enc_out), reinterpret_cast<uint64_t*>(elements_out)));
  }
  void msm_segmented_resident(int dev, void* stream, const Encoding* points, const Fr* scalars, const uint64_t* offsets,
                              const uint64_t* offsets_dev, size_t n, Encoding* enc_out, Element* elements_out, uint8_t* status) {
    check(d377_batch_segmented_msm_encoded_resident(ctx_, dev, stream, reinterpret_cast<const uint8_t*>(points),
                                                    reinterpret_cast<const uint8_t*>(scalars), offsets, offsets_dev, n,
                                                    reinterpret_cast<uint8_t*>(enc_out), reinterpret_cast<uint64_t*>(elements_out), status));
  }
  /// CurveGroup::normalize_batch (src/ark_curve/element.rs:74-81): affine (x, y) as 4 Montgomery limbs each
  std::vector<std::array<uint64_t, 8>> normalize_batch(const std::vector<Element>& p) {
    std::vector<std::array<uint64_t, 8>> out(p.size());
    check(d377_batch_to_affine(ctx_, u64(p), p.size(), reinterpret_cast<uint64_t*>(out.data())));
    return out;
  }
  /// decompress then compress: Ok(e) has e == input (tests/encoding.rs:97-107)
  std::vector<Result<Encoding>> roundtrip(const std::vector<Encoding>& encs) {
    std::vector<Encoding> out(encs.size());
    std::vector<uint8_t> st(encs.size());
    check(d377_batch_roundtrip(ctx_, u8(encs), encs.size(), u8m(out), st.data()));
    return results(out, st);
  }
  static Element identity() { Element e; d377_identity(e.xyzt.data()); return e; }     // Element::IDENTITY
  static Element generator() { Element e; d377_generator(e.xyzt.data()); return e; }   // Element::GENERATOR
  d377_ctx* raw() { return ctx_; }

 private:
  template <class T> static const uint8_t* u8(const std::vector<T>& v) { return reinterpret_cast<const uint8_t*>(v.data()); }
  template <class T> static uint8_t* u8m(std::vector<T>& v) { return reinterpret_cast<uint8_t*>(v.data()); }
  static const uint64_t* u64(const std::vector<Element>& v) { return reinterpret_cast<const uint64_t*>(v.data()); }
  static void check(int rc) { if (rc != D377_OK) throw DeviceError(rc); }
  Element msm_short_host(const void* scalars, int scalar_bytes, size_t n, const std::vector<Element>& points, Encoding* encoding) {
    if (n != points.size()) throw std::invalid_argument("length mismatch");
    Element out;
    Encoding enc;
    check(d377_msm_short(ctx_, u64(points), static_cast<const uint8_t*>(scalars), scalar_bytes, n, enc.b.data(), out.xyzt.data()));
    if (encoding) *encoding = enc;
    return out;
  }
  template <class T>
  static std::vector<Result<T>> results(const std::vector<T>& v, const std::vector<uint8_t>& st) {
    std::vector<Result<T>> r(v.size());
    for (size_t i = 0; i < v.size(); ++i) r[i] = {st[i] == 0, v[i], EncodingError::InvalidEncoding};
    return r;
  }
  template <class T>
  static std::vector<T> values(const std::vector<Result<T>>& v) {
    std::vector<T> r(v.size());
    for (size_t i = 0; i < v.size(); ++i) r[i] = v[i].value;
    return r;
  }
  d377_ctx* ctx_ = nullptr;
  friend class FixedBases;
  std::mutex fixed_mu_;
  std::vector<FixedBases*> fixed_;                          // the live FixedBases of this Engine
  void rebind(FixedBases* from, FixedBases* to) {
    std::lock_guard<std::mutex> lock(fixed_mu_);
    for (auto& p : fixed_)
      if (p == from) p = to;
  }
  void forget(FixedBases* fb) {
    std::lock_guard<std::mutex> lock(fixed_mu_);
    for (size_t i = 0; i < fixed_.size(); ++i)
      if (fixed_[i] == fb) { fixed_.erase(fixed_.begin() + (std::ptrdiff_t)i); break; }
  }
};

inline FixedBases::FixedBases(FixedBases&& o) noexcept : eng_(o.eng_), h_(o.h_), m_(o.m_) {
  if (eng_) eng_->rebind(&o, this);
  o.eng_ = nullptr; o.h_ = 0;
}
inline FixedBases& FixedBases::operator=(FixedBases&& o) noexcept {
  if (this != &o) {
    reset();
    eng_ = o.eng_; h_ = o.h_; m_ = o.m_;
    if (eng_) eng_->rebind(&o, this);
    o.eng_ = nullptr; o.h_ = 0;
  }
  return *this;
}
inline d377_ctx* FixedBases::ctx() const { return eng_ ? eng_->ctx_ : nullptr; }
inline void FixedBases::reset() {
  if (eng_) {
    eng_->forget(this);
    if (h_) d377_fixed_bases_destroy(eng_->ctx_, h_);
  }
  eng_ = nullptr; h_ = 0;
}

}  // namespace decaf377
