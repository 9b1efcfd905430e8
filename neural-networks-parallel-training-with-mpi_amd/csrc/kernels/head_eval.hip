// Forward-only output layer for evaluation and prediction: logits, per-row loss and per-row
// argmax of a head of ANY shape, without dlogits, dZ or a gradient (head.hip / head_general.hip
// are the training heads; evaluating through them stores a dZ nobody reads and runs a
// weight-gradient kernel whose result is discarded).
//
// One wave per row, RPW rows per wave-iteration, HW waves per block (head_fwd_kernel's pattern):
// the rows are loaded ONCE into registers with unconditional clamped loads (a chunk past the
// row's end becomes zeros), then the outputs are walked in tiles of `to` <= 16 outputs.  A tile's fp32 weights sit
// in LDS -- for 8-wide lane chunks in head.hip's conflict-free [o][2][in/8][4] image, for the
// scalar form (fp32 rows of any width / alignment: one feature per lane-chunk) as plain [o][in],
// where consecutive lanes read consecutive words.  `to` is the largest count whose image fits
// 64 KiB (16 up to 1,024 features, 2 at 8,192).  The RPW x to partial products of a tile are
// reduced by ONE batched butterfly; across tiles a row carries the online-softmax state (running
// max, sum of exponentials, the label's logit), the running argmax and the two MSE sums, so any
// `out` is one pass over the activations with no rows x out round trip.  A head of one tile
// (every out <= 16 head of <= 1,024 features) stages W once per block; more tiles restage per
// block-iteration (the rows, not the weights, are what stays in registers).
//
// The label is only compared with the output index (as int64), never used as one.  The argmax
// is torch.argmax's: the first index of the maximum, a NaN counting as the maximum.
//
// Forms: the VALU kernel below (any shape), and a matrix-core kernel for the multi-output heads
// of 512 / 1,024 bf16 features (MNIST), further down.
//
// Metrics: every row's fp32 loss / hit / absolute error is added in double by its wave in
// row order, the waves of a block in wave order, and one finalize block sums the per-block
// partials in a fixed tree (grad_sumsq / clip_finalize's scheme, optim.hip).  No atomics; the
// grid is a function of the shape and the form (operand alignment picks the form): same inputs,
// same bits.
#include "common.h"
#include "kernels.h"
#include "head_common.h"

#include <algorithm>

namespace nnmpi {

namespace {

constexpr int EV_LDS_FLOATS = 16384;   // 64 KiB weight tile
constexpr int EV_MAX_BLOCKS = 256;     // one block per CU
constexpr int EV_MAX_IN = 8192;

struct EvalArgs {
  const void* a;
  int lda, rows, in;
  const float* W;
  const float* b;
  int out;
  const float* y;
  const int64_t* labels;
  int loss;
  float* logits;
  int ldl;
  int* pred;
  double* part;   // [blocks][3]: loss, correct, abs error (null: no metrics)
  int to;         // outputs per tile
  int nit;        // block-iterations: ceil(rows / (HW * RPW))
};

// E: features per lane-chunk (8: 16-byte loads, in % 8 == 0, aligned rows; 1: scalar form).
// CMAX: lane-chunks per lane (64 * CMAX * E >= in).  OUTM: the compile-time bound of `to`.
template <typename TA, int E, int CMAX, int RPW, int HW, int OUTM>
__global__ void __launch_bounds__(64 * HW) head_eval_kernel(EvalArgs p) {
  extern __shared__ __attribute__((aligned(16))) float wl[];   // the tile's weight image
  __shared__ double red[HW][3];
  constexpr int NT = 64 * HW;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // uniform: row indices stay scalar
  const int in = p.in, out = p.out, rows = p.rows, loss = p.loss;
  const int nch = E == 8 ? in >> 3 : in;   // lane-chunks per row
  const TA* A = reinterpret_cast<const TA*>(p.a);
  // lane-chunk c of this lane: clamped for the (unconditional) loads, the values of a chunk past
  // the row's end replaced by zeros (recomputed where used: the scalar form has 128 of them)
  auto chc = [&](int c) { return min(c * 64 + lane, nch - 1); };
  auto live = [&](int c) { return c * 64 + lane < nch; };
  const int ntiles = (out + p.to - 1) / p.to;
  double wloss = 0.0, wcorr = 0.0, wabs = 0.0;

  for (int it = blockIdx.x; it < p.nit; it += gridDim.x) {
    const int r0 = (it * HW + w) * RPW;
    float av[RPW][CMAX][E];
    long long labv[RPW];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
      const int r = min(r0 + q, rows - 1);   // clamped: loads stay unconditional
#pragma unroll
      for (int c = 0; c < CMAX; ++c) {
        if constexpr (E == 8) load8<TA>(A + (long long)r * p.lda + chc(c) * 8, av[q][c]);
        else av[q][c][0] = (float)A[(long long)r * p.lda + chc(c)];
#pragma unroll
        for (int e = 0; e < E; ++e) av[q][c][e] = live(c) ? av[q][c][e] : 0.f;
      }
      labv[q] = loss == LOSS_XENT ? (long long)p.labels[r] : -1ll;
    }
    // per-row state carried across the output tiles
    float mx[RPW], se[RPW], zl[RPW], best[RPW], sq[RPW], ab[RPW];
    int besti[RPW];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
      mx[q] = -INFINITY; se[q] = 0.f; zl[q] = 0.f; best[q] = -INFINITY; besti[q] = -1;
      sq[q] = 0.f; ab[q] = 0.f;
    }

    for (int t = 0; t < ntiles; ++t) {
      const int t0 = t * p.to, tn = min(p.to, out - t0);
      if (ntiles > 1 || it == (int)blockIdx.x) {   // uniform per block
        __syncthreads();                           // the previous tile's readers are done
        const float* Wt = p.W + (long long)t0 * in;
        for (int i = tid; i < tn * in; i += NT) {
          int d = i;
          if constexpr (E == 8) {
            const int o = i / in, k = i - o * in;
            d = o * in + ((k >> 2) & 1) * (nch * 4) + (k >> 3) * 4 + (k & 3);
          }
          wl[d] = Wt[i];
        }
        __syncthreads();
      }
      // an offset the compiler cannot see through keeps the LDS weight reads inside the row loop
      // (hoisted, a 10 x 1024 head wants 320 VGPRs of weights: head.hip)
      int wo = 0;
      asm volatile("" : "+v"(wo));
      const float* wlo = wl + wo;
      float bias[OUTM];
#pragma unroll
      for (int o = 0; o < OUTM; ++o) bias[o] = p.b[t0 + min(o, tn - 1)];
      float part[RPW][OUTM];
#pragma unroll
      for (int q = 0; q < RPW; ++q)
#pragma unroll
        for (int o = 0; o < OUTM; ++o) part[q][o] = 0.f;
#pragma unroll
      for (int o = 0; o < OUTM; ++o) {
        if (o >= tn) continue;   // uniform: no work for the padding outputs
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
          if constexpr (E == 8) {
            const float* wr = wlo + o * in + chc(c) * 4;
            const float4 w0 = *reinterpret_cast<const float4*>(wr);
            const float4 w1 = *reinterpret_cast<const float4*>(wr + nch * 4);
#pragma unroll
            for (int q = 0; q < RPW; ++q) {
              const float tq = av[q][c][0] * w0.x + av[q][c][1] * w0.y + av[q][c][2] * w0.z +
                               av[q][c][3] * w0.w + av[q][c][4] * w1.x + av[q][c][5] * w1.y +
                               av[q][c][6] * w1.z + av[q][c][7] * w1.w;
              part[q][o] += tq;
            }
          } else {
            const float wv = wlo[o * in + chc(c)];
#pragma unroll
            for (int q = 0; q < RPW; ++q) part[q][o] += av[q][c][0] * wv;
          }
        }
      }
      // one batched butterfly for the tile
#pragma unroll
      for (int sh = 32; sh >= 1; sh >>= 1)
#pragma unroll
        for (int q = 0; q < RPW; ++q)
#pragma unroll
          for (int o = 0; o < OUTM; ++o)
            if (o < tn) part[q][o] += __shfl_xor(part[q][o], sh, 64);

#pragma unroll
      for (int q = 0; q < RPW; ++q) {
        const bool valid = (r0 + q) < rows;
        const int r = min(r0 + q, rows - 1);
        float lg[OUTM];
#pragma unroll
        for (int o = 0; o < OUTM; ++o) lg[o] = part[q][o] + bias[o];
        // running argmax, torch.argmax's rule: first maximum, a NaN is the maximum
#pragma unroll
        for (int o = 0; o < OUTM; ++o) {
          if (o >= tn) continue;
          // (selects, not a branch: !(z <= best) is "z > best or z is NaN" for an ordered best)
          const float z = lg[o];
          const bool take = (besti[q] < 0) | ((best[q] == best[q]) & !(z <= best[q]));
          best[q] = take ? z : best[q];
          besti[q] = take ? t0 + o : besti[q];
        }
        if (loss == LOSS_XENT) {
          float tm = -INFINITY;
#pragma unroll
          for (int o = 0; o < OUTM; ++o) if (o < tn) tm = fmaxf(tm, lg[o]);
          const float nm = fmaxf(mx[q], tm);
          const float ref = nm == -INFINITY ? 0.f : nm;
          float s = se[q] * __expf(mx[q] - ref);
#pragma unroll
          for (int o = 0; o < OUTM; ++o) {
            if (o >= tn) continue;
            s += __expf(lg[o] - ref);
            zl[q] = (long long)(t0 + o) == labv[q] ? lg[o] : zl[q];   // compared, never an index
          }
          se[q] = s;
          mx[q] = nm;
        } else if (loss == LOSS_MSE) {
#pragma unroll
          for (int o = 0; o < OUTM; ++o) {
            if (o >= tn) continue;
            const float d = lg[o] - p.y[(long long)r * out + t0 + o];
            sq[q] += d * d;
            ab[q] += fabsf(d);
          }
        }
        if (p.logits != nullptr) {
          float my = 0.f;
#pragma unroll
          for (int o = 0; o < OUTM; ++o) if (lane == o) my = lg[o];
          if (valid && lane < tn) p.logits[(long long)r * p.ldl + t0 + lane] = my;
        }
      }
    }

#pragma unroll
    for (int q = 0; q < RPW; ++q) {
      if ((r0 + q) >= rows) continue;
      if (loss == LOSS_XENT) {
        wloss += (double)((mx[q] + __logf(se[q])) - zl[q]);
        wcorr += (long long)besti[q] == labv[q] ? 1.0 : 0.0;
      } else if (loss == LOSS_MSE) {
        wloss += (double)sq[q];
        wabs += (double)ab[q];
      }
      if (p.pred != nullptr && lane == 0) p.pred[r0 + q] = besti[q];
    }
  }

  if (p.part != nullptr) {
    if (lane == 0) {
      red[w][0] = wloss;
      red[w][1] = wcorr;
      red[w][2] = wabs;
    }
    __syncthreads();
    if (tid == 0) {   // wave partials in wave order
      double l = red[0][0], c = red[0][1], a = red[0][2];
#pragma unroll
      for (int k = 1; k < HW; ++k) {
        l += red[k][0];
        c += red[k][1];
        a += red[k][2];
      }
      double* dst = p.part + (long long)blockIdx.x * 3;
      dst[0] = l;
      dst[1] = c;
      dst[2] = a;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Matrix-core form for the multi-output heads the training step runs on head_mfma_kernel (bf16
// rows, in = 512 / 1,024, 2 <= out <= 16, 16-byte aligned W): the VALU form above took 34.8 us on
// the 8,192 x 1,024 x 10 MNIST head against 11.9 + 4.5 us for the training head and its combine
// (rocprofv3, docs/PERF.md section 7), all of it butterflies and LDS weight reads.  Same layout as
// head_mfma_kernel: a block of 4 waves takes one 16-row group at a time, wave w the w-th quarter
// of the features on v_mfma_f32_16x16x4_f32 (exact fp32 products and sums), W in LDS as fp32
// [16][in] with 16-byte chunk c of row n at c ^ (n & 15); the four partial tiles are summed
// through LDS in wave order.  Wave 0 then holds the group's logits (lane: row lane & 15, outputs
// 4 (lane >> 4) .. + 3) and finishes softmax / MSE / argmax with two cross-lane steps each; its
// rows' results are added in double per lane, the 16 row lanes in lane order at the end.
// ------------------------------------------------------------------------------------------
constexpr int EM_WAVES = 4;
constexpr int EM_NONE = 0x7fffffff;   // "no candidate yet" index of the argmax merge

// (v2, i2) replaces (v1, i1): torch.argmax's order -- a NaN beats every number, equal ranks go to
// the lower index
__device__ __forceinline__ void argmax_merge(float& v1, int& i1, float v2, int i2) {
  const bool n1 = v1 != v1, n2 = v2 != v2;
  const bool higher = (n2 & !n1) | (!n1 & !n2 & (v2 > v1));
  const bool same = (n1 & n2) | (!n1 & !n2 & (v2 == v1));
  const bool take = (i2 != EM_NONE) & ((i1 == EM_NONE) | higher | (same & (i2 < i1)));
  v1 = take ? v2 : v1;
  i1 = take ? i2 : i1;
}

template <int Q>
__global__ void __launch_bounds__(64 * EM_WAVES) head_eval_mfma_kernel(EvalArgs p) {
  extern __shared__ __attribute__((aligned(16))) float ml[];   // W image [16][in] + partials
  __shared__ double red[16][3];
  constexpr int in = 4 * Q;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int out = p.out, rows = p.rows, loss = p.loss;
  const bf16* A = reinterpret_cast<const bf16*>(p.a);
  const int r = lane & 15, g = lane >> 4;
  const int ngroups = (rows + 15) / 16;
  // this wave's quarter of a row group: 8 features per 32-chunk and lane (row r, column group g)
  auto load_rows = [&](bf16x8 (&xs)[Q / 32], int grp) {
    const int rowc = min(grp * 16 + r, rows - 1);
    const bf16* ar = A + (long long)rowc * p.lda + w * Q + g * 8;
#pragma unroll
    for (int c = 0; c < Q / 32; ++c) xs[c] = *reinterpret_cast<const bf16x8*>(ar + c * 32);
  };
  bf16x8 cur[Q / 32], nxt[Q / 32];
  load_rows(cur, blockIdx.x);          // in flight while the W image is built
  constexpr int NV = 16 * in / 4 / (64 * EM_WAVES);
  f32x4 wv[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int i4 = j * 64 * EM_WAVES + tid, n = i4 / (in / 4), k = (i4 % (in / 4)) * 4;
    wv[j] = n < out ? *reinterpret_cast<const f32x4*>(p.W + n * in + k) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int i4 = j * 64 * EM_WAVES + tid, n = i4 / (in / 4), k = (i4 % (in / 4)) * 4;
    *reinterpret_cast<f32x4*>(ml + mh_off(n, k, in)) = wv[j];
  }
  f32x4* part = reinterpret_cast<f32x4*>(ml + 16 * in);   // [4 waves][64 lanes]
  __syncthreads();
  float bias[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bias[j] = (4 * g + j) < out ? p.b[4 * g + j] : 0.f;
  double wloss = 0.0, wcorr = 0.0, wabs = 0.0;

  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    load_rows(nxt, min(grp + (int)gridDim.x, ngroups - 1));   // past the end: never used
    const int row = grp * 16 + r;
    const bool valid = row < rows;
    const int rowc = min(row, rows - 1);
    long long lab = -1;
    float yv[4] = {0.f, 0.f, 0.f, 0.f};
    if (w == 0) {   // targets of the rows wave 0 finishes, in flight under the products
      if (loss == LOSS_XENT) lab = (long long)p.labels[rowc];
      if (loss == LOSS_MSE) {
#pragma unroll
        for (int j = 0; j < 4; ++j) yv[j] = p.y[(long long)rowc * out + min(4 * g + j, out - 1)];
      }
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < Q / 32; ++c) {
      const int k = w * Q + c * 32 + g * 8;
      const bf16x8 xv = cur[c];
      const f32x4 w0 = *reinterpret_cast<const f32x4*>(ml + mh_off(r, k, in));
      const f32x4 w1 = *reinterpret_cast<const f32x4*>(ml + mh_off(r, k + 4, in));
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[e], (float)xv[e], acc, 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[e], (float)xv[e + 4], acc, 0, 0, 0);
    }
    part[w * 64 + lane] = acc;
    __syncthreads();
    if (w == 0) {
      f32x4 z = part[lane];
#pragma unroll
      for (int ww = 1; ww < EM_WAVES; ++ww) z += part[ww * 64 + lane];
      float bv = -INFINITY;
      int bi = EM_NONE;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        z[j] += bias[j];
        argmax_merge(bv, bi, z[j], (4 * g + j) < out ? 4 * g + j : EM_NONE);
      }
#pragma unroll
      for (int sh = 16; sh <= 32; sh <<= 1) {
        const float ov = __shfl_xor(bv, sh, 64);
        const int oi = __shfl_xor(bi, sh, 64);
        argmax_merge(bv, bi, ov, oi);
      }
      float row_loss = 0.f, row_abs = 0.f;
      if (loss == LOSS_XENT) {
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) if (4 * g + j < out) mx = fmaxf(mx, z[j]);
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float ref = mx == -INFINITY ? 0.f : mx;
        float se = 0.f, picked = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (4 * g + j < out) se += __expf(z[j] - ref);
          picked += (long long)(4 * g + j) == lab ? z[j] : 0.f;   // compared, never an index
        }
        se += __shfl_xor(se, 16, 64);
        se += __shfl_xor(se, 32, 64);
        picked += __shfl_xor(picked, 16, 64);
        picked += __shfl_xor(picked, 32, 64);
        row_loss = (mx + __logf(se)) - picked;
      } else if (loss == LOSS_MSE) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float d = (4 * g + j) < out ? z[j] - yv[j] : 0.f;
          row_loss += d * d;
          row_abs += fabsf(d);
        }
        row_loss += __shfl_xor(row_loss, 16, 64);
        row_loss += __shfl_xor(row_loss, 32, 64);
        row_abs += __shfl_xor(row_abs, 16, 64);
        row_abs += __shfl_xor(row_abs, 32, 64);
      }
      if (valid) {
        if (p.logits != nullptr) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (4 * g + j < out) p.logits[(long long)row * p.ldl + 4 * g + j] = z[j];
        }
        if (g == 0) {
          if (loss == LOSS_XENT) {
            wloss += (double)row_loss;
            wcorr += (long long)bi == lab ? 1.0 : 0.0;
          } else if (loss == LOSS_MSE) {
            wloss += (double)row_loss;
            wabs += (double)row_abs;
          }
          if (p.pred != nullptr) p.pred[row] = bi;
        }
      }
    }
    __syncthreads();   // the partials are rewritten by the next group
#pragma unroll
    for (int c = 0; c < Q / 32; ++c) cur[c] = nxt[c];
  }

  if (p.part != nullptr) {
    if (tid < 16) {
      red[tid][0] = wloss;
      red[tid][1] = wcorr;
      red[tid][2] = wabs;
    }
    __syncthreads();
    if (tid == 0) {   // the 16 row lanes in lane order
      double l = red[0][0], c = red[0][1], a = red[0][2];
#pragma unroll
      for (int k = 1; k < 16; ++k) {
        l += red[k][0];
        c += red[k][1];
        a += red[k][2];
      }
      double* dst = p.part + (long long)blockIdx.x * 3;
      dst[0] = l;
      dst[1] = c;
      dst[2] = a;
    }
  }
}

bool eval_mfma_ok(const void* a, int a_bf16, int lda, int in, int out, const float* W) {
  return a_bf16 && (in == 512 || in == 1024) && out >= 2 && out <= HEAD_OMAX && lda % 8 == 0 &&
         (reinterpret_cast<uintptr_t>(a) & 15) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0;
}

template <int Q>
hipError_t eval_launch_mfma(const EvalArgs& p, int blocks, hipStream_t s) {
  const size_t smem = (size_t)(16 * p.in + EM_WAVES * 64 * 4) * sizeof(float);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)head_eval_mfma_kernel<Q>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    attr = true;
  }
  hipLaunchKernelGGL(head_eval_mfma_kernel<Q>, dim3(blocks), dim3(64 * EM_WAVES), smem, s, p);
  return hipGetLastError();
}

// One block: the per-block partials in a fixed tree, then metrics = (or +=) [loss_sum, correct,
// abs_err_sum, rows].
__global__ void __launch_bounds__(256) head_eval_finalize_kernel(const double* __restrict__ part,
                                                                 int nparts, double rows,
                                                                 double* __restrict__ metrics,
                                                                 int accumulate) {
  __shared__ double red[256][3];
  const int t = threadIdx.x;
  double v[3] = {0.0, 0.0, 0.0};
  for (int i = t; i < nparts; i += 256)
#pragma unroll
    for (int j = 0; j < 3; ++j) v[j] += part[(long long)i * 3 + j];
#pragma unroll
  for (int j = 0; j < 3; ++j) red[t][j] = v[j];
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (t < st)
#pragma unroll
      for (int j = 0; j < 3; ++j) red[t][j] += red[t + st][j];
    __syncthreads();
  }
  if (t < 4) {
    const double add = t < 3 ? red[0][t] : rows;
    metrics[t] = accumulate ? metrics[t] + add : add;
  }
}

// Block geometry by lane-chunks per row (nch = in / 8, scalar form: in).  The 8-wide forms are
// head_launch_c's: 16 / 8 waves for rows of <= 512 / 1,024 features (several waves per SIMD keep
// the chip's row loads in flight), 4 for wider rows (their registers only fit at low occupancy).
struct EvalForm { int cmax, rpw, hw; };

EvalForm eval_form(int nch, bool vec) {
  if (vec) {
    if (nch <= 64) return {1, 2, 16};
    if (nch <= 128) return {2, 4, 8};
    if (nch <= 256) return {4, 2, 4};
    return {16, 1, 4};
  }
  if (nch <= 64) return {1, 4, 8};
  if (nch <= 512) return {8, 2, 8};
  return {128, 1, 4};
}

bool eval_vec(const void* a, int a_bf16, int lda, int in) {
  const int e = a_bf16 ? 8 : 4;   // elements per 16 bytes
  return in % 8 == 0 && lda % e == 0 && (reinterpret_cast<uintptr_t>(a) & 15) == 0;
}

int eval_blocks(int rows, int in, int out) {
  // (the forms' geometries differ; all are bounded by the same cap, and the workspace is sized
  // for the largest count)
  int most = std::max(1, std::min((rows + 15) / 16, EV_MAX_BLOCKS));
  for (int vec = 0; vec < 2; ++vec) {
    if (vec && in % 8) continue;
    const EvalForm f = eval_form(vec ? in / 8 : in, vec != 0);
    const int per = f.hw * f.rpw;
    most = std::max(most, std::min((rows + per - 1) / per, EV_MAX_BLOCKS));
  }
  return most;
}

template <typename TA, int E, int CMAX, int RPW, int HW>
hipError_t eval_launch(EvalArgs p, hipStream_t s) {
  constexpr int per = HW * RPW;
  p.nit = (p.rows + per - 1) / per;
  const int blocks = std::min(p.nit, EV_MAX_BLOCKS);
  const size_t smem = (size_t)p.to * p.in * sizeof(float);
  if (p.out == 1)
    hipLaunchKernelGGL((head_eval_kernel<TA, E, CMAX, RPW, HW, 1>), dim3(blocks), dim3(64 * HW), smem, s, p);
  else
    hipLaunchKernelGGL((head_eval_kernel<TA, E, CMAX, RPW, HW, HEAD_OMAX>), dim3(blocks), dim3(64 * HW), smem, s, p);
  return hipGetLastError();
}

template <typename TA>
hipError_t eval_launch_vec(const EvalArgs& p, hipStream_t s) {
  const int nch = p.in / 8;
  if (nch <= 64) return eval_launch<TA, 8, 1, 2, 16>(p, s);
  if (nch <= 128) return eval_launch<TA, 8, 2, 4, 8>(p, s);
  if (nch <= 256) return eval_launch<TA, 8, 4, 2, 4>(p, s);
  return eval_launch<TA, 8, 16, 1, 4>(p, s);
}

}  // namespace

int head_eval_form(const void* a, int a_bf16, int lda, int in, int out, const float* W) {
  if (eval_mfma_ok(a, a_bf16, lda, in, out, W)) return 2;
  return eval_vec(a, a_bf16, lda, in) ? 1 : 0;
}

size_t head_eval_workspace_bytes(int rows, int in, int out) {
  return (size_t)eval_blocks(std::max(rows, 0), std::max(in, 1), out) * 3 * sizeof(double);
}

hipError_t head_eval(const void* a, int a_bf16, int lda, int rows, int in, const float* W,
                     const float* b, int out, const float* y, const int64_t* labels, int loss,
                     float* logits_out, int ldl, int* pred_out, double* metrics, int accumulate,
                     float* ws, hipStream_t s) {
  if (W == nullptr || b == nullptr) return hipErrorInvalidValue;
  if (rows < 0 || in < 1 || out < 1 || in > EV_MAX_IN || lda < in) return hipErrorInvalidValue;
  if (loss != LOSS_MSE && loss != LOSS_XENT && loss != -1) return hipErrorInvalidValue;
  // (an empty batch has nothing to point at: rows == 0 reads neither the rows nor the targets)
  if (rows > 0 && (a == nullptr || (loss == LOSS_MSE && y == nullptr) ||
                   (loss == LOSS_XENT && labels == nullptr))) return hipErrorInvalidValue;
  if (logits_out != nullptr && ldl < out) return hipErrorInvalidValue;
  if (metrics != nullptr && (ws == nullptr || (reinterpret_cast<uintptr_t>(ws) & 7) != 0)) return hipErrorInvalidValue;
  const bool vec = eval_vec(a, a_bf16, lda, in);
  if (a_bf16 && !vec) return hipErrorInvalidValue;   // bf16 rows: in % 8 == 0, 16-byte aligned
  double* part = metrics != nullptr ? reinterpret_cast<double*>(ws) : nullptr;
  int nparts = 0;
  if (rows > 0) {
    EvalArgs p;
    p.a = a; p.lda = lda; p.rows = rows; p.in = in;
    p.W = W; p.b = b; p.out = out;
    p.y = y; p.labels = labels; p.loss = loss;
    p.logits = logits_out; p.ldl = ldl; p.pred = pred_out; p.part = part;
    p.to = std::max(1, std::min(std::min(out, HEAD_OMAX), EV_LDS_FLOATS / in));
    p.nit = 0;
    hipError_t e;
    if (eval_mfma_ok(a, a_bf16, lda, in, out, W)) {
      nparts = std::min((rows + 15) / 16, EV_MAX_BLOCKS);
      e = in == 512 ? eval_launch_mfma<128>(p, nparts, s) : eval_launch_mfma<256>(p, nparts, s);
    } else if (vec) {
      e = a_bf16 ? eval_launch_vec<bf16>(p, s) : eval_launch_vec<float>(p, s);
    } else {
      const EvalForm f = eval_form(in, false);
      e = f.cmax == 1 ? eval_launch<float, 1, 1, 4, 8>(p, s)
        : f.cmax == 8 ? eval_launch<float, 1, 8, 2, 8>(p, s)
                      : eval_launch<float, 1, 128, 1, 4>(p, s);
    }
    if (e != hipSuccess) return e;
    if (nparts == 0) {
      const EvalForm f = eval_form(vec ? in / 8 : in, vec);
      const int per = f.hw * f.rpw;
      nparts = std::min((rows + per - 1) / per, EV_MAX_BLOCKS);
    }
  }
  if (metrics != nullptr && (rows > 0 || !accumulate)) {
    hipLaunchKernelGGL(head_eval_finalize_kernel, dim3(1), dim3(256), 0, s, part, nparts,
                       (double)rows, metrics, accumulate);
    return hipGetLastError();
  }
  return hipSuccess;
}

}  // namespace nnmpi
