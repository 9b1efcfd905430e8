// Inverted dropout of a hidden layer's activations and its backward, the mask never stored: it
// is a pure function of (seed, pass, rank, layer, logical element index) through the
// counter-based generator Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as
// 1, 2, 3", SC'11), so the backward regenerates it, a replayed graph draws a fresh one every
// replay (seed and pass are read from device memory), and a CPU reference reproduces it bit for
// bit (ops/torch_ops.py).
//
// Mask.  Element e = r * H + c of a [rows][H] matrix (LOGICAL: the row stride plays no part)
// takes word e & 3 of the Philox call with
//   counter = (g lo32, g hi32, pass, (rank << 8) | layer),  g = e >> 2,   key = (seed lo32, hi32)
// and is kept iff word >= T, T = min(2^32 - 1, round(p * 2^32)) from the host.
//   dropout_fwd: d = kept ? T(float(a) * scale) : +0          scale = float(1 / (1 - p)), host
//   dropout_bwd: dd = kept ? T(float(dd) * scale * act'(a)) : +0, in place; a is the UNDROPPED
//                saved activation.  With g = float(dd) * scale (fp32): relu a > 0 ? g : 0, none g;
//                tanh: dd * scale * (1 - a^2) formed in double (fma(-a, a, 1)) and rounded once.
//
// Work split.  A row is cut into the chunks of rowwise.h (8 bf16 / 4 fp32, or 1 fp32 in the
// scalar form).  H is a multiple of the chunk, so chunk q of
// the matrix holds the logical elements q * VEC ..: a chunk is exactly two (bf16), one (fp32) or
// a quarter (scalar: the call of g = q >> 2, word q & 3 -- a call group may straddle two rows)
// Philox calls, and the counter needs q alone.  Nothing is reduced over a row, so the grid is a
// flat stride loop over chunks; a row is only an address: (row, column chunk) of a thread's next
// chunk follow from the previous one by adding the grid stride's (quotient, remainder) by H /
// VEC, computed on the host -- no division in the loop.  Every thread holds DROP_INFLIGHT chunks
// per trip and issues all of their loads before the first Philox round, so the integer work of
// chunk k (10 rounds = 20 mul_hi / mul_lo pairs per call) runs under the latency of the rest.
// The grid depends on the element count alone.  64-bit element indices; rows * H < 2^34.
#include "rowwise.h"

namespace nnmpi {
namespace {

constexpr int DROP_THREADS = 256;
constexpr int DROP_INFLIGHT = 4;     // chunks per thread and trip
constexpr int DROP_MAX_BLOCKS = 2048;   // 8 blocks on each of 256 CUs
constexpr long long DROP_MAX_ELEMS = 1ll << 34;

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

// Philox4x32-10: ten rounds, the key advanced by the Weyl constants between them.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t (&w)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
    const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// The VEC mask words of chunk q.
template <int VEC>
__device__ __forceinline__ void chunk_words(unsigned long long q, uint32_t pass, uint32_t tag,
                                            uint32_t k0, uint32_t k1, uint32_t (&w)[VEC]) {
  if constexpr (VEC == 8) {
    uint32_t lo[4], hi[4];
    const unsigned long long g = q * 2;
    philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), pass, tag, k0, k1, lo);
    philox4x32_10((uint32_t)(g + 1), (uint32_t)((g + 1) >> 32), pass, tag, k0, k1, hi);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w[i] = lo[i];
      w[4 + i] = hi[i];
    }
  } else if constexpr (VEC == 4) {
    philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), pass, tag, k0, k1, w);
  } else {
    uint32_t t[4];
    const unsigned long long g = q >> 2;
    philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), pass, tag, k0, k1, t);
    const int i = (int)(q & 3);
    w[0] = i == 0 ? t[0] : i == 1 ? t[1] : i == 2 ? t[2] : t[3];   // (selects: no indexed array)
  }
}

// x: the forward's operand a (BWD: the gradient dd, out == x: in place; y the saved activation).
// n chunks of VEC elements, C = H / VEC per row; (srow, scol) = the grid stride / and % C.
template <typename T, int VEC, bool BWD, int ACT>
__global__ __launch_bounds__(DROP_THREADS) void dropout_kernel(
    const T* x, long long ldx, const T* __restrict__ y, long long ldy, T* out, long long ldo,
    const int* __restrict__ state, unsigned long long n, unsigned C, unsigned long long srow, unsigned scol, uint32_t thr, float scale, uint32_t tag) {
#pragma clang fp contract(off)
  typedef typename RowVec<T, VEC>::type V;
  const uint32_t k0 = (uint32_t)state[0], k1 = (uint32_t)state[1], pass = (uint32_t)state[2];
  const unsigned tid = blockIdx.x * DROP_THREADS + threadIdx.x;
  const unsigned long long stride = (unsigned long long)gridDim.x * DROP_THREADS;
  unsigned long long row = tid / C;
  unsigned col = tid % C;
  for (unsigned long long q = tid; q < n; q += DROP_INFLIGHT * stride) {
    V vx[DROP_INFLIGHT], vy[DROP_INFLIGHT];
    long long oo[DROP_INFLIGHT];
    bool ok[DROP_INFLIGHT];
#pragma unroll
    for (int k = 0; k < DROP_INFLIGHT; ++k) {
      ok[k] = q + k * stride < n;
      const long long cc = (long long)col * VEC;
      oo[k] = (long long)row * ldo + cc;
      V tx = {}, ty = {};
      if (ok[k]) {
        tx = *reinterpret_cast<const V*>(x + (long long)row * ldx + cc);
        if constexpr (BWD && ACT != ACT_NONE)
          ty = *reinterpret_cast<const V*>(y + (long long)row * ldy + cc);
      }
      vx[k] = tx;
      vy[k] = ty;
      row += srow;
      col += scol;
      if (col >= C) {
        col -= C;
        ++row;
      }
    }
#pragma unroll
    for (int k = 0; k < DROP_INFLIGHT; ++k) {
      if (!ok[k]) continue;
      uint32_t w[VEC];
      chunk_words<VEC>(q + k * stride, pass, tag, k0, k1, w);
      V o;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        float g = elem(vx[k], i) * scale;
        if constexpr (BWD && ACT == ACT_RELU) g = elem(vy[k], i) > 0.f ? g : 0.f;
        if constexpr (BWD && ACT == ACT_TANH) {
          // three fp32 roundings (dd * scale, 1 - a^2, their product) are up to 1.9 fp32 ulp
          // from the exact value: the product is formed in double and rounded once
          const double a = (double)elem(vy[k], i);
          g = (float)(((double)elem(vx[k], i) * (double)scale) * fma(-a, a, 1.0));
        }
        put(o, i, w[i] >= thr ? g : 0.f);
      }
      *reinterpret_cast<V*>(out + oo[k]) = o;
    }
  }
}

__global__ void dropout_tick_kernel(int* __restrict__ state) { state[2] += 1; }

// dropout's own arguments (the operands: row_check, rowwise.h)
bool drop_args_ok(int rows, int H, float scale, int layer, int rank) {
  return (long long)rows * H < DROP_MAX_ELEMS && layer >= 0 && layer <= 255 && rank >= 0 &&
         rank < (1 << 24) && scale >= 1.f && scale * 0.f == 0.f;   // (NaN, inf: refused)
}

template <typename T, int VEC, bool BWD, int ACT>
hipError_t drop_launch(const void* x, long long ldx, const void* y, long long ldy, void* out,
                       long long ldo, const int* state, int rows, int H, unsigned thr, float scale,
                       int layer, int rank, hipStream_t s) {
  const unsigned C = (unsigned)(H / VEC);
  const unsigned long long n = (unsigned long long)rows * C;
  const unsigned long long per = (unsigned long long)DROP_THREADS * DROP_INFLIGHT;
  unsigned long long blocks = (n + per - 1) / per;
  if (blocks > DROP_MAX_BLOCKS) blocks = DROP_MAX_BLOCKS;
  const unsigned long long stride = blocks * DROP_THREADS;
  dropout_kernel<T, VEC, BWD, ACT><<<dim3((unsigned)blocks), dim3(DROP_THREADS), 0, s>>>(
      static_cast<const T*>(x), ldx, static_cast<const T*>(y), ldy, static_cast<T*>(out), ldo,
      state, n, C, stride / C, (unsigned)(stride % C), thr, scale,
      ((uint32_t)rank << 8) | (uint32_t)layer);
  return hipGetLastError();
}

}  // namespace

hipError_t dropout_fwd(const void* a, long long lda, void* d, long long ldd, const int* state,
                       int is_bf16, int rows, int H, unsigned T, float scale, int layer, int rank,
                       hipStream_t s) {
  int vec = 0;
  const hipError_t e = row_check(is_bf16, a, lda, d, ldd, state, rows, H,
                                 drop_args_ok(rows, H, scale, layer, rank), &vec);
  if (e != hipSuccess || rows == 0) return e;
  return row_pick_vec(vec, [&](auto t, auto v) {
    return drop_launch<decltype(t), decltype(v)::value, false, ACT_NONE>(
        a, lda, a, lda, d, ldd, state, rows, H, T, scale, layer, rank, s);
  });
}

hipError_t dropout_bwd(void* dd, long long ldd, const void* a, long long lda, const int* state,
                       int is_bf16, int rows, int H, unsigned T, float scale, int act, int layer,
                       int rank, hipStream_t s) {
  int vec = 0;
  const hipError_t e = row_check(is_bf16, dd, ldd, a, lda, state, rows, H,
                                 act_known(act) && drop_args_ok(rows, H, scale, layer, rank), &vec);
  if (e != hipSuccess || rows == 0) return e;
  return row_pick_act(act, [&](auto ac) {
    return row_pick_vec(vec, [&](auto t, auto v) {
      return drop_launch<decltype(t), decltype(v)::value, true, decltype(ac)::value>(
          dd, ldd, a, lda, dd, ldd, state, rows, H, T, scale, layer, rank, s);
    });
  });
}

hipError_t dropout_tick(int* state, hipStream_t s) {
  if (!state) return hipErrorInvalidValue;
  dropout_tick_kernel<<<dim3(1), dim3(1), 0, s>>>(state);
  return hipGetLastError();
}

}  // namespace nnmpi
