// GPU harness of the field multiplier streams (decaf377_amd/csrc/fe_asm.inc, reached through fq29.hpp and fqs29.hpp), built
// and run by tests/test_field_streams.py:
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -fPIC -shared tests/cpp/field_streams.hip -o build/field_streams.so
// One lane per row of nine 32-bit limbs.  Each lane computes a product through the public function (on the device: the
// instruction stream) and through the *_ref statement the stream is generated from (the compiler's translation), so the
// test can compare the two with each other and with its own model on Python integers.  The linear operations around the
// streams (fe_sub, fe_sub_nc, fe_carry, fe_canon; fe_sub, fe_carry, fe_unsigned on fes) are returned as the device computes
// them.  Test infrastructure only: every entry point does its own allocation and copies and returns a HIP error as a
// non-zero code.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../decaf377_amd/csrc/fqs29.hpp"

using namespace d377;

namespace {

constexpr int BLOCK = 64;                 // one wave per block: a size that is no multiple of 64 ends in a partial wave
constexpr int MAX_ROWS = 1 << 20;
constexpr int N_PRODUCT_OPS = 8, N_LINEAR_OPS = 7;

// product ops: 0 fe_mul, 1 fe_mul_strict, 2 fe_sqr, 3 fe_sqr_strict, 4 fe_sqr2x (fe); 5 fe_mul, 6 fe_sqr, 7 fe_sqr2x (fes)
template <int OP> using field_of = typename std::conditional<(OP < 5), fe, fes>::type;

template <class F>
__device__ __forceinline__ F row_load(const uint32_t* p) {
  F r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.l[i] = (decltype(r.l[0] + 0))p[i];
  return r;
}
template <class F>
__device__ __forceinline__ void row_store(uint32_t* p, const F& r) {
#pragma unroll
  for (int i = 0; i < NL; ++i) p[i] = (uint32_t)r.l[i];
}

// the public function: on the device, the stream of fe_asm.inc
template <int OP, class F>
__device__ __forceinline__ F op_stream(const F& a, const F& b) {
  if constexpr (OP == 0 || OP == 5) return fe_mul(a, b);
  else if constexpr (OP == 1) return fe_mul_strict(a, b);
  else if constexpr (OP == 2 || OP == 6) return fe_sqr(a);
  else if constexpr (OP == 3) return fe_sqr_strict(a);
  else return fe_sqr2x(a);
}
// the statement it is generated from
template <int OP, class F>
__device__ __forceinline__ F op_ref(const F& a, const F& b) {
  if constexpr (OP == 0) return fe_mul_ref<false>(a, b);
  else if constexpr (OP == 1) return fe_mul_ref<true>(a, b);
  else if constexpr (OP == 2) return fe_sqr_ref<false, false>(a);
  else if constexpr (OP == 3) return fe_sqr_ref<true, false>(a);
  else if constexpr (OP == 4) return fe_sqr_ref<false, true>(a);
  else if constexpr (OP == 5) return fes_mul_ref<false, false>(a, b);
  else if constexpr (OP == 6) return fes_mul_ref<false, true>(a, a);
  else return fes_mul_ref<true, true>(a, a);
}

// PRED: only the lanes the mode selects run the product (1: odd rows; 2: a test on the row's data); the others return
// without writing, so their output rows keep what the host put there.  A comparison made before the product is consumed
// after it (flag): a lane mask that is live across the stream.
template <int OP, bool PRED>
__global__ void __launch_bounds__(BLOCK) k_product(const uint32_t* a, const uint32_t* b, int n, int mode, uint32_t* got,
                                                   uint32_t* want, uint32_t* flag) {
  using F = field_of<OP>;
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t* pa = a + (size_t)NL * i;
  const uint32_t* pb = b + (size_t)NL * i;
  if (PRED) {
    const bool on = mode == 1 ? (i & 1) != 0 : ((pa[0] ^ (uint32_t)i) & 3u) == 1u;
    if (!on) return;
  }
  const F x = row_load<F>(pa), y = row_load<F>(pb);
  const bool lt = pa[1] < pb[2];
  const F g = op_stream<OP>(x, y);
  row_store(got + (size_t)NL * i, g);
  if (PRED) flag[i] = lt ? 1u : 2u;
  const F w = op_ref<OP>(x, y);
  row_store(want + (size_t)NL * i, w);
}

// The op inside a loop and under register pressure: x = op(x (+|-) u, y) with two more live products u and v, folded into
// the result at the end.  x, u and v start as products of the rows, so every operand of the loop is a product or a sum or
// difference of two.  fe: the op's operand is the lazy sum x + u (2 x^2 takes carried limbs: x alone); fes: the difference
// x - u, limbs of either sign.  y is the row itself (carried width).  mul / sqr: the side chains' product and squaring.
template <int OP, bool REF, class F>
__device__ __forceinline__ F chain(const F& a, const F& b, int iters) {
  auto mul = [](const F& p, const F& q) { if constexpr (REF) return op_ref<(OP < 5 ? 0 : 5)>(p, q); else return fe_mul(p, q); };
  auto sqr = [](const F& p) { if constexpr (REF) return op_ref<(OP < 5 ? 2 : 6)>(p, p); else return fe_sqr(p); };
  F x = sqr(a), y = b, u = mul(a, b), v = sqr(b);
#pragma unroll 1
  for (int t = 0; t < iters; ++t) {
    F in;
    if constexpr (OP == 4) in = x;
    else if constexpr (OP < 5) in = fe_add(x, u);
    else in = fe_sub(x, u);
    if constexpr (REF) x = op_ref<OP>(in, y); else x = op_stream<OP>(in, y);
    u = mul(u, x);
    if constexpr (OP < 5) v = sqr(fe_add(v, x)); else v = sqr(fe_sub(v, x));
  }
  return fe_sub(fe_add(x, u), v);
}
template <int OP>
__global__ void __launch_bounds__(BLOCK) k_chain(const uint32_t* a, const uint32_t* b, int n, int iters, uint32_t* got, uint32_t* want) {
  using F = field_of<OP>;
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const F x = row_load<F>(a + (size_t)NL * i), y = row_load<F>(b + (size_t)NL * i);
  row_store(got + (size_t)NL * i, chain<OP, false>(x, y, iters));
  row_store(want + (size_t)NL * i, chain<OP, true>(x, y, iters));
}

// linear ops: 0 fe_sub, 1 fe_sub_nc, 2 fe_carry, 3 fe_canon (fe); 4 fe_carry, 5 fe_sub, 6 fe_unsigned (fes)
__global__ void __launch_bounds__(BLOCK) k_linear(int op, const uint32_t* a, const uint32_t* b, int n, uint32_t* out) {
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t* pa = a + (size_t)NL * i;
  const uint32_t* pb = b + (size_t)NL * i;
  uint32_t* po = out + (size_t)NL * i;
  if (op < 4) {
    const fe x = row_load<fe>(pa), y = row_load<fe>(pb);
    row_store(po, op == 0 ? fe_sub(x, y) : op == 1 ? fe_sub_nc(x, y) : op == 2 ? fe_carry(x) : fe_canon(x));
  } else {
    const fes x = row_load<fes>(pa), y = row_load<fes>(pb);
    if (op == 4) row_store(po, fe_carry(x));
    else if (op == 5) row_store(po, fe_sub(x, y));
    else row_store(po, fe_unsigned(x));
  }
}

struct DevRows {                            // n rows of nine words on the device, freed on every return path
  uint32_t* p = nullptr;
  ~DevRows() { if (p) (void)hipFree(p); }
};

#define CK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) { fprintf(stderr, "field_streams: %s: %s\n", #e, hipGetErrorString(e_)); return (int)e_; } } while (0)
#define EACH_OP(X) case 0: X(0); break; case 1: X(1); break; case 2: X(2); break; case 3: X(3); break; \
                   case 4: X(4); break; case 5: X(5); break; case 6: X(6); break; default: X(7); break;

int run_product(int op, int mode, const uint32_t* a, const uint32_t* b, int n, uint32_t* got, uint32_t* want, uint32_t* flag) {
  if (op < 0 || op >= N_PRODUCT_OPS || mode < 0 || mode > 2 || n <= 0 || n > MAX_ROWS || !a || !b || !got || !want || (mode && !flag)) return -1;
  const size_t bytes = (size_t)n * NL * sizeof(uint32_t), fbytes = (size_t)n * sizeof(uint32_t);
  DevRows da, db, dg, dw, df;
  CK(hipMalloc(&da.p, bytes)); CK(hipMalloc(&db.p, bytes)); CK(hipMalloc(&dg.p, bytes)); CK(hipMalloc(&dw.p, bytes)); CK(hipMalloc(&df.p, fbytes));
  CK(hipMemcpy(da.p, a, bytes, hipMemcpyHostToDevice)); CK(hipMemcpy(db.p, b, bytes, hipMemcpyHostToDevice));
  // the caller's sentinel goes in and must come back from every lane that did not run
  CK(hipMemcpy(dg.p, got, bytes, hipMemcpyHostToDevice)); CK(hipMemcpy(dw.p, want, bytes, hipMemcpyHostToDevice));
  if (mode) CK(hipMemcpy(df.p, flag, fbytes, hipMemcpyHostToDevice));
  const dim3 grid((n + BLOCK - 1) / BLOCK), block(BLOCK);
#define LAUNCH(OP) do { if (mode) hipLaunchKernelGGL((k_product<OP, true>), grid, block, 0, 0, da.p, db.p, n, mode, dg.p, dw.p, df.p); \
                        else hipLaunchKernelGGL((k_product<OP, false>), grid, block, 0, 0, da.p, db.p, n, mode, dg.p, dw.p, df.p); } while (0)
  switch (op) { EACH_OP(LAUNCH) }
#undef LAUNCH
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(got, dg.p, bytes, hipMemcpyDeviceToHost)); CK(hipMemcpy(want, dw.p, bytes, hipMemcpyDeviceToHost));
  if (mode) CK(hipMemcpy(flag, df.p, fbytes, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

// got, want: n rows each; row i = op(a_i, b_i) through the stream / through its statement (the squarers ignore b)
extern "C" int streams_product(int op, const uint32_t* a, const uint32_t* b, int n, uint32_t* got, uint32_t* want) {
  return run_product(op, 0, a, b, n, got, want, nullptr);
}
// mode 1: odd rows only; mode 2: rows with ((a_i[0] ^ i) & 3) == 1.  got, want (n rows) and flag (n words) are read and
// written: a row that does not run keeps what the caller put there; one that runs also sets flag_i = a_i[1] < b_i[2] ? 1 : 2.
extern "C" int streams_predicated(int op, int mode, const uint32_t* a, const uint32_t* b, int n, uint32_t* got, uint32_t* want, uint32_t* flag) {
  if (mode != 1 && mode != 2) return -1;
  return run_product(op, mode, a, b, n, got, want, flag);
}
extern "C" int streams_chain(int op, const uint32_t* a, const uint32_t* b, int n, int iters, uint32_t* got, uint32_t* want) {
  if (op < 0 || op >= N_PRODUCT_OPS || n <= 0 || n > MAX_ROWS || iters < 0 || iters > 4096 || !a || !b || !got || !want) return -1;
  const size_t bytes = (size_t)n * NL * sizeof(uint32_t);
  DevRows da, db, dg, dw;
  CK(hipMalloc(&da.p, bytes)); CK(hipMalloc(&db.p, bytes)); CK(hipMalloc(&dg.p, bytes)); CK(hipMalloc(&dw.p, bytes));
  CK(hipMemcpy(da.p, a, bytes, hipMemcpyHostToDevice)); CK(hipMemcpy(db.p, b, bytes, hipMemcpyHostToDevice));
  CK(hipMemset(dg.p, 0, bytes)); CK(hipMemset(dw.p, 0xFF, bytes));
  const dim3 grid((n + BLOCK - 1) / BLOCK), block(BLOCK);
#define LAUNCH(OP) hipLaunchKernelGGL((k_chain<OP>), grid, block, 0, 0, da.p, db.p, n, iters, dg.p, dw.p)
  switch (op) { EACH_OP(LAUNCH) }
#undef LAUNCH
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(got, dg.p, bytes, hipMemcpyDeviceToHost)); CK(hipMemcpy(want, dw.p, bytes, hipMemcpyDeviceToHost));
  return 0;
}
extern "C" int streams_linear(int op, const uint32_t* a, const uint32_t* b, int n, uint32_t* out) {
  if (op < 0 || op >= N_LINEAR_OPS || n <= 0 || n > MAX_ROWS || !a || !b || !out) return -1;
  const size_t bytes = (size_t)n * NL * sizeof(uint32_t);
  DevRows da, db, dout;
  CK(hipMalloc(&da.p, bytes)); CK(hipMalloc(&db.p, bytes)); CK(hipMalloc(&dout.p, bytes));
  CK(hipMemcpy(da.p, a, bytes, hipMemcpyHostToDevice)); CK(hipMemcpy(db.p, b, bytes, hipMemcpyHostToDevice));
  CK(hipMemset(dout.p, 0xA5, bytes));
  hipLaunchKernelGGL(k_linear, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, 0, op, da.p, db.p, n, dout.p);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost));
  return 0;
}
