// Layer / RMS normalisation of a hidden layer's pre-activations, without learned scale or shift
// (torch.nn.LayerNorm(H, elementwise_affine=False) and its RMS counterpart), fused with the
// activation that follows it, and its backward.  Over one row z[0..H):
//   layer: mu = mean(z), rstd = 1 / sqrt(mean((z - mu)^2) + eps), x = (z - mu) * rstd
//          dz = rstd * (dn - mean(dn) - x * mean(dn * x))
//   rms:   mu = 0,       rstd = 1 / sqrt(mean(z^2) + eps),        x = z * rstd
//          dz = rstd * (dn - x * mean(dn * x))
// norm_act_fwd writes a = act(x) and the row's (mu, rstd); norm_bwd turns dL/dx (what the head or
// linear_dgrad left in the layer's dZ buffer: they apply act' through the saved a) into dL/dz in
// place, recomputing x from the saved z and the stored statistics with the forward's expression
// (norm_x), so both directions see the same x bit for bit.
//
// Work split.  A row is cut into the chunks of rowwise.h (8 bf16 / 4 fp32, or 1 fp32 in the
// scalar-load form); C = H / chunk is what selects the form:
//   wave form  (C <= 256: bf16 H <= 2048, fp32 H <= 1024, scalar H <= 256).  Every lane holds
//     NORM_INFLIGHT = 4 chunks, all loaded before the first is used.  C <= 64: one chunk per row
//     and lane, a row owned by the 2^lg >= C adjacent lanes of a wave (64 >> lg rows side by side)
//     and four such row groups in flight -- an 8-wide row still moves 16 bytes per lane, 256 rows
//     per wave.  C <= 128 / 256: 2 / 4 chunks per lane, 2 / 1 rows in flight.
//   block form (wider, up to 8,192 features): one 256-thread block per row, 2 / 4 / 8 (scalar: 8 /
//     32) chunks per thread, the waves' partials combined through LDS in wave order.
// The row is read once and stays in registers (bf16 packed as loaded).  Statistics are two-pass
// (the mean, then the centred squares), summed in double and stored as fp32; x is computed from
// the stored fp32 values.  Every row sum is a fixed-order xor butterfly
// over the row's lanes (then the wave-order LDS sum): no atomics, and the lanes that share a row
// depend on H alone, so the result does not depend on the row count or the grid.  The backward's
// two sums (dn, dn * x) of all rows in flight go through ONE butterfly.
#include "rowwise.h"

namespace nnmpi {
namespace {

constexpr int NORM_THREADS = 256;
constexpr int NORM_WAVES = NORM_THREADS / WAVE;
constexpr int NORM_INFLIGHT = 4;   // chunks per lane of the wave form

// Which rows and chunks a thread holds.  Wave form: U row groups in flight, a row on 2^lg lanes;
// block form: the block's row, chunks NORM_THREADS apart.
template <int NC, bool BLOCK>
struct NormMap {
  static constexpr int U = BLOCK ? 1 : NORM_INFLIGHT / NC;
  static constexpr int CSTEP = BLOCK ? NORM_THREADS : WAVE;
  long long row[U];
  int c0, lpr;
  bool lead;   // writes the row's statistics
  __device__ __forceinline__ explicit NormMap(int lg) {
    if constexpr (BLOCK) {
      lpr = WAVE;
      row[0] = blockIdx.x;
      c0 = threadIdx.x;
    } else {
      lpr = 1 << lg;
      const int lane = threadIdx.x & (WAVE - 1);
      const long long wave = (long long)blockIdx.x * NORM_WAVES + (threadIdx.x >> 6);
#pragma unroll
      for (int u = 0; u < U; ++u) row[u] = ((wave * U + u) << (6 - lg)) + (lane >> lg);
      c0 = lane & (lpr - 1);
    }
    lead = c0 == 0;
  }
};

// v[i] = the sum of v[i] over the row's lanes: xor butterfly over the lpr lanes of the row, widest
// step first; block form: then the waves' partials, added in wave order by every thread.
template <bool BLOCK, int N>
__device__ __forceinline__ void row_sum(double (&v)[N], int lpr) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    if (o < lpr) {   // (uniform)
#pragma unroll
      for (int i = 0; i < N; ++i) v[i] += __shfl_xor(v[i], o, WAVE);
    }
  }
  if constexpr (BLOCK) {
    __shared__ double part[NORM_WAVES * N];
    const int w = threadIdx.x >> 6;
    __syncthreads();   // the readers of the previous sum are done
    if ((threadIdx.x & (WAVE - 1)) == 0) {
#pragma unroll
      for (int i = 0; i < N; ++i) part[w * N + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double t = part[i];
#pragma unroll
      for (int q = 1; q < NORM_WAVES; ++q) t += part[q * N + i];
      v[i] = t;
    }
  }
}

// The normalised element both directions use: an exact function of the saved z and the STORED
// fp32 statistics, rounded once.
__device__ __forceinline__ float norm_x(float z, float mu, float rstd) {
  return (float)(((double)z - (double)mu) * (double)rstd);
}

template <typename T, int VEC, int NC, bool BLOCK, int NORM, int ACT>
__global__ __launch_bounds__(NORM_THREADS) void norm_act_fwd_kernel(
    const T* __restrict__ z, long long ldz, T* __restrict__ a, long long lda,
    float* __restrict__ stats, int rows, int H, int lg, float eps) {
#pragma clang fp contract(off)
  typedef typename RowVec<T, VEC>::type V;
  typedef NormMap<NC, BLOCK> Map;
  constexpr int U = Map::U;
  const Map m(lg);
  const int C = H / VEC;
  V v[U][NC];
  bool ok[U][NC];
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int c = m.c0 + k * Map::CSTEP;
      ok[u][k] = m.row[u] < rows && c < C;
      V t = {};
      if (ok[u][k]) t = *reinterpret_cast<const V*>(z + m.row[u] * ldz + (long long)c * VEC);
      v[u][k] = t;
    }
  }
  // row sums in double (a memory-bound kernel has the cycles): mu and rstd are the fp32 roundings
  // of sums that carry no summation error of their own
  double acc[U];
  float mu[U], rs[U];
#pragma unroll
  for (int u = 0; u < U; ++u) acc[u] = 0.0;
  if constexpr (NORM == NORM_LAYER) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int k = 0; k < NC; ++k) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[u] += (double)elem(v[u][k], i);   // (not held: zero)
      }
    }
    row_sum<BLOCK>(acc, m.lpr);
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = acc[u] / (double)H;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const double mean = acc[u];
    mu[u] = (float)mean;
    double q = 0.0;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const double d = (double)elem(v[u][k], i) - mean;
        q = ok[u][k] ? fma(d, d, q) : q;
      }
    }
    acc[u] = q;
  }
  row_sum<BLOCK>(acc, m.lpr);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    rs[u] = (float)(1.0 / sqrt(acc[u] / (double)H + (double)eps));
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      if (!ok[u][k]) continue;
      V o;
#pragma unroll
      for (int i = 0; i < VEC; ++i)
        put(o, i, act_fwd_t<ACT>(norm_x(elem(v[u][k], i), mu[u], rs[u])));
      *reinterpret_cast<V*>(a + m.row[u] * lda + (long long)(m.c0 + k * Map::CSTEP) * VEC) = o;
    }
    if (m.lead && m.row[u] < rows) {
      stats[2 * m.row[u]] = mu[u];
      stats[2 * m.row[u] + 1] = rs[u];
    }
  }
}

template <typename T, int VEC, int NC, bool BLOCK, int NORM>
__global__ __launch_bounds__(NORM_THREADS) void norm_bwd_kernel(
    T* __restrict__ dn, long long ldd, const T* __restrict__ z, long long ldz,
    const float* __restrict__ stats, int rows, int H, int lg) {
#pragma clang fp contract(off)
  typedef typename RowVec<T, VEC>::type V;
  typedef NormMap<NC, BLOCK> Map;
  constexpr int U = Map::U;
  constexpr int NS = NORM == NORM_LAYER ? 2 : 1;   // sums per row: (dn,) dn * x
  const Map m(lg);
  const int C = H / VEC;
  V g[U][NC], v[U][NC];
  bool ok[U][NC];
  float mu[U], rs[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const bool live = m.row[u] < rows;
    mu[u] = live ? stats[2 * m.row[u]] : 0.f;
    rs[u] = live ? stats[2 * m.row[u] + 1] : 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int c = m.c0 + k * Map::CSTEP;
      ok[u][k] = live && c < C;
      V tg = {}, tz = {};
      if (ok[u][k]) {
        tg = *reinterpret_cast<const V*>(dn + m.row[u] * ldd + (long long)c * VEC);
        tz = *reinterpret_cast<const V*>(z + m.row[u] * ldz + (long long)c * VEC);
      }
      g[u][k] = tg;
      v[u][k] = tz;
    }
  }
  double sum[U * NS];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) {   // (a chunk not held: dn = 0 adds nothing to either sum)
        const double gi = (double)elem(g[u][k], i);
        s1 += gi;
        s2 = fma(gi, (double)norm_x(elem(v[u][k], i), mu[u], rs[u]), s2);
      }
    }
    sum[u * NS + NS - 1] = s2;
    if constexpr (NS == 2) sum[u * NS] = s1;
  }
  row_sum<BLOCK>(sum, m.lpr);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const double m2 = sum[u * NS + NS - 1] / (double)H;
    const double m1 = NS == 2 ? sum[u * NS] / (double)H : 0.0;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      if (!ok[u][k]) continue;
      V o;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const double x = (double)norm_x(elem(v[u][k], i), mu[u], rs[u]);
        put(o, i, (float)((double)rs[u] * (((double)elem(g[u][k], i) - m1) - x * m2)));
      }
      *reinterpret_cast<V*>(dn + m.row[u] * ldd + (long long)(m.c0 + k * Map::CSTEP) * VEC) = o;
    }
  }
}

// ---- host side: which form a row width takes, and the template dispatch -----------------------
struct NormPlan {
  int nc;       // chunks per thread
  bool block;   // block form
  int lg;       // wave form: log2 of the lanes that share a row
  unsigned grid;
};

bool norm_plan(int rows, int H, int vec, NormPlan& p) {
  const int C = H / vec;
  p.block = C > WAVE * NORM_INFLIGHT;
  p.lg = 6;
  if (!p.block) {
    p.nc = C <= WAVE ? 1 : C <= 2 * WAVE ? 2 : 4;
    if (p.nc == 1) {
      p.lg = 0;
      while ((1 << p.lg) < C) ++p.lg;
    }
    const long long per_wave = (long long)(NORM_INFLIGHT / p.nc) * (WAVE >> p.lg);
    const long long waves = (rows + per_wave - 1) / per_wave;
    p.grid = (unsigned)((waves + NORM_WAVES - 1) / NORM_WAVES);
    return true;
  }
  const int per = (C + NORM_THREADS - 1) / NORM_THREADS;
  p.nc = vec == 1 ? (per <= 8 ? 8 : 32) : per <= 2 ? 2 : per <= 4 ? 4 : 8;
  p.grid = (unsigned)rows;
  return per <= p.nc;
}

// f(IC<NC>, bool_constant<BLOCK>) for the plan's form; only the forms a (T, VEC) pair can reach
// are instantiated (bf16 stops at 4 chunks per thread, only the scalar form reaches 32)
template <typename T, int VEC, typename F>
hipError_t norm_pick_form(const NormPlan& p, F&& f) {
  if (!p.block) {
    if (p.nc == 1) return f(IC<1>{}, std::false_type{});
    if (p.nc == 2) return f(IC<2>{}, std::false_type{});
    return f(IC<4>{}, std::false_type{});
  }
  if constexpr (VEC != 1) {
    if (p.nc == 2) return f(IC<2>{}, std::true_type{});
    if (p.nc == 4) return f(IC<4>{}, std::true_type{});
  }
  if constexpr (std::is_same<T, float>::value) {
    if (p.nc == 8) return f(IC<8>{}, std::true_type{});
  }
  if constexpr (VEC == 1) {
    if (p.nc == 32) return f(IC<32>{}, std::true_type{});
  }
  return hipErrorInvalidValue;
}

template <typename F>
hipError_t norm_pick_kind(int norm, F&& f) {
  if (norm == NORM_LAYER) return f(IC<NORM_LAYER>{});
  if (norm == NORM_RMS) return f(IC<NORM_RMS>{});
  return hipErrorInvalidValue;
}

// The front both launchers share: the operand check (rowwise.h; ``op_ok``: the caller's own
// arguments), the plan, and f(T(), IC<VEC>, IC<NC>, bool_constant<BLOCK>, IC<NORM>, plan) for
// what they select.  No rows: success, nothing launched.
template <typename F>
hipError_t norm_launch(int is_bf16, const void* p0, long long ld0, const void* p1, long long ld1,
                       const float* stats, int rows, int H, int norm, bool op_ok, F&& f) {
  int vec = 0;
  NormPlan p;
  op_ok = op_ok && (norm == NORM_LAYER || norm == NORM_RMS);
  const hipError_t e = row_check(is_bf16, p0, ld0, p1, ld1, stats, rows, H, op_ok, &vec);
  if (e != hipSuccess || rows == 0) return e;
  if (!norm_plan(rows, H, vec, p)) return hipErrorInvalidValue;
  return row_pick_vec(vec, [&](auto t, auto v) {
    return norm_pick_form<decltype(t), decltype(v)::value>(p, [&](auto nc, auto blk) {
      return norm_pick_kind(norm, [&](auto kind) { return f(t, v, nc, blk, kind, p); });
    });
  });
}

}  // namespace

hipError_t norm_act_fwd(const void* z, long long ldz, void* a, long long lda, float* stats,
                        int is_bf16, int rows, int H, int norm, int act, float eps,
                        hipStream_t s) {
  const bool op_ok = act_known(act) && eps >= 0.f;   // (NaN: refused)
  return norm_launch(is_bf16, z, ldz, a, lda, stats, rows, H, norm, op_ok,
                     [&](auto t, auto v, auto nc, auto blk, auto kind, const NormPlan& p) {
    typedef decltype(t) T;
    return row_pick_act(act, [&](auto ac) {
      norm_act_fwd_kernel<T, decltype(v)::value, decltype(nc)::value, decltype(blk)::value,
                          decltype(kind)::value, decltype(ac)::value>
          <<<dim3(p.grid), dim3(NORM_THREADS), 0, s>>>(static_cast<const T*>(z), ldz,
                                                       static_cast<T*>(a), lda, stats, rows, H,
                                                       p.lg, eps);
      return hipGetLastError();
    });
  });
}

hipError_t norm_bwd(void* dn, long long ldd, const void* z, long long ldz, const float* stats,
                    int is_bf16, int rows, int H, int norm, hipStream_t s) {
  return norm_launch(is_bf16, dn, ldd, z, ldz, stats, rows, H, norm, true,
                     [&](auto t, auto v, auto nc, auto blk, auto kind, const NormPlan& p) {
    typedef decltype(t) T;
    norm_bwd_kernel<T, decltype(v)::value, decltype(nc)::value, decltype(blk)::value,
                    decltype(kind)::value>
        <<<dim3(p.grid), dim3(NORM_THREADS), 0, s>>>(static_cast<T*>(dn), ldd,
                                                     static_cast<const T*>(z), ldz, stats, rows, H,
                                                     p.lg);
    return hipGetLastError();
  });
}

}  // namespace nnmpi
