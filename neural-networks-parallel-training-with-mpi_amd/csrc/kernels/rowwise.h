// What a row-chunk kernel over [rows][H] row-strided matrices needs (norm.hip, dropout.hip): a
// row is cut into CHUNKS of 16 bytes -- 8 bf16 or 4 fp32 -- or, in the scalar form that takes
// fp32 rows of any width and alignment, of one fp32.  The chunk's vector type and element access,
// the width rule, the launchers' operand check (plain host code) and the template dispatch.
#pragma once
#include <type_traits>

#include "common.h"

namespace nnmpi {

constexpr int ROW_MAX_H = 8192;   // features per row

template <typename T, int VEC> struct RowVec;
template <> struct RowVec<bf16, 8> { typedef bf16x8 type; };
template <> struct RowVec<float, 4> { typedef f32x4 type; };
template <> struct RowVec<float, 1> { typedef float type; };

__device__ __forceinline__ float elem(const bf16x8& v, int i) { return (float)v[i]; }
__device__ __forceinline__ float elem(const f32x4& v, int i) { return v[i]; }
__device__ __forceinline__ float elem(const float& v, int) { return v; }
__device__ __forceinline__ void put(bf16x8& v, int i, float x) { v[i] = (bf16)x; }
__device__ __forceinline__ void put(f32x4& v, int i, float x) { v[i] = x; }
__device__ __forceinline__ void put(float& v, int, float x) { v = x; }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the byte ranges of two [rows][H] operands (rows > 0) of es-byte elements intersect
inline bool overlap(const void* p0, long long ld0, const void* p1, long long ld1, int rows, int H,
                    int es) {
  const char* a = static_cast<const char*>(p0);
  const char* b = static_cast<const char*>(p1);
  const long long na = ((rows - 1) * ld0 + H) * es, nb = ((rows - 1) * ld1 + H) * es;
  return a < b + nb && b < a + na;
}

// Elements per chunk for two row-strided operands: 8 (bf16), 4 / 1 (fp32); 0: not taken (bf16
// rows that are not H % 8 == 0, 16-byte aligned with strides % 8 == 0)
inline int row_vec(int is_bf16, int H, const void* p0, long long ld0, const void* p1,
                   long long ld1) {
  const int v = is_bf16 ? 8 : 4;
  const bool ok = H % v == 0 && ld0 % v == 0 && ld1 % v == 0 && aligned16(p0) && aligned16(p1);
  return ok ? v : (is_bf16 ? 0 : 1);
}

inline bool act_known(int act) { return act == ACT_NONE || act == ACT_RELU || act == ACT_TANH; }

// The check every launcher runs first (``op_ok``: the op's own arguments are valid; ``aux``: its
// third device operand).  Every argument error is hipErrorInvalidValue; rows == 0 with valid
// arguments is hipSuccess whatever the pointers (the caller launches nothing); null operands,
// overlap and an untakeable bf16 row are refused only with rows > 0.  *vec: the width to run.
inline hipError_t row_check(int is_bf16, const void* p0, long long ld0, const void* p1,
                            long long ld1, const void* aux, int rows, int H, bool op_ok,
                            int* vec) {
  *vec = 0;
  if (!op_ok || rows < 0 || H <= 0 || H > ROW_MAX_H || ld0 < H || ld1 < H)
    return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  if (!p0 || !p1 || !aux) return hipErrorInvalidValue;
  if (overlap(p0, ld0, p1, ld1, rows, H, is_bf16 ? 2 : 4)) return hipErrorInvalidValue;
  *vec = row_vec(is_bf16, H, p0, ld0, p1, ld1);
  return *vec == 0 ? hipErrorInvalidValue : hipSuccess;
}

template <int I> using IC = std::integral_constant<int, I>;

// f(T(), IC<VEC>) for the chunk width row_check chose
template <typename F>
hipError_t row_pick_vec(int vec, F&& f) {
  if (vec == 8) return f(bf16(), IC<8>{});
  if (vec == 4) return f(float(), IC<4>{});
  return f(float(), IC<1>{});
}

template <typename F>
hipError_t row_pick_act(int act, F&& f) {
  if (act == ACT_NONE) return f(IC<ACT_NONE>{});
  if (act == ACT_RELU) return f(IC<ACT_RELU>{});
  if (act == ACT_TANH) return f(IC<ACT_TANH>{});
  return hipErrorInvalidValue;
}

}  // namespace nnmpi
