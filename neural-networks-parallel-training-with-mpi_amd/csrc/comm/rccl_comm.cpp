#include <cstdlib>
#include "knobs.h"
#include "rccl_comm.h"
#include "kernels/kernels.h"

#include <algorithm>
#include <cstring>
#include <stdexcept>

namespace nnmpi {

#define HIP_THROW(x)                                                                     \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess)                                                                \
      throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e_) + " at " + \
                               __FILE__ + ":" + std::to_string(__LINE__));               \
  } while (0)

#define NCCL_THROW(x)                                                                    \
  do {                                                                                   \
    ncclResult_t r_ = (x);                                                               \
    if (r_ != ncclSuccess)                                                               \
      throw std::runtime_error(std::string("RCCL error: ") + ncclGetErrorString(r_) + " at " + \
                               __FILE__ + ":" + std::to_string(__LINE__));               \
  } while (0)

static ncclDataType_t to_nccl(int dtype) {
  switch (dtype) {
    case 0: return ncclFloat32;
    case 1: return ncclBfloat16;
    case 2: return ncclFloat64;
    case 3: return ncclInt64;
    case 4: return ncclInt32;
    case 5: return ncclUint8;
    default: throw std::runtime_error("unsupported dtype code");
  }
}

static size_t dtype_size(int dtype) {
  switch (dtype) {
    case 0: return 4;
    case 1: return 2;
    case 2: return 8;
    case 3: return 8;
    case 4: return 4;
    case 5: return 1;
    default: return 0;
  }
}

static ncclRedOp_t to_op(int op) {
  switch (op) {
    case 0: return ncclSum;
    case 1: return ncclAvg;
    case 2: return ncclMax;
    case 3: return ncclMin;
    default: throw std::runtime_error("unsupported reduction op");
  }
}

std::string RcclComm::get_unique_id() {
  ncclUniqueId id;
  NCCL_THROW(ncclGetUniqueId(&id));
  return std::string(id.internal, sizeof(id.internal));
}

RcclComm::RcclComm(const std::string& uid, int nranks, int rank, int device)
    : nranks_(nranks), rank_(rank), device_(device) {
  if (uid.size() != sizeof(ncclUniqueId)) throw std::runtime_error("bad ncclUniqueId size");
  ncclUniqueId id;
  std::memcpy(id.internal, uid.data(), sizeof(id.internal));
  HIP_THROW(hipSetDevice(device));
  NCCL_THROW(ncclCommInitRank(&comm_, nranks, id, rank));
}

RcclComm::~RcclComm() {
  if (comm_ && !aborted_) ncclCommDestroy(comm_);
}

void RcclComm::allreduce(void* buf, size_t count, int dtype, int op, hipStream_t s) {
  NCCL_THROW(ncclAllReduce(buf, buf, count, to_nccl(dtype), to_op(op), comm_, s));
}

void RcclComm::broadcast(void* buf, size_t count, int dtype, int root, hipStream_t s) {
  NCCL_THROW(ncclBroadcast(buf, buf, count, to_nccl(dtype), root, comm_, s));
}

void RcclComm::reduce(void* buf, size_t count, int dtype, int op, int root, hipStream_t s) {
  NCCL_THROW(ncclReduce(buf, buf, count, to_nccl(dtype), to_op(op), root, comm_, s));
}

void RcclComm::allgather(const void* sendbuf, void* recvbuf, size_t count, int dtype, hipStream_t s) {
  NCCL_THROW(ncclAllGather(sendbuf, recvbuf, count, to_nccl(dtype), comm_, s));
}

void RcclComm::reduce_scatter(const void* sendbuf, void* recvbuf, size_t recvcount, int dtype,
                              int op, hipStream_t s) {
  NCCL_THROW(ncclReduceScatter(sendbuf, recvbuf, recvcount, to_nccl(dtype), to_op(op), comm_, s));
}

void RcclComm::scatterv(const void* sendbuf, const std::vector<long long>& counts,
                        const std::vector<long long>& displs, void* recvbuf, int dtype, int root,
                        hipStream_t s) {
  if ((int)counts.size() != nranks_ || (int)displs.size() != nranks_)
    throw std::runtime_error("scatterv: counts/displs must have one entry per rank");
  const size_t es = dtype_size(dtype);
  const ncclDataType_t dt = to_nccl(dtype);
  NCCL_THROW(ncclGroupStart());
  if (rank_ == root) {
    for (int r = 0; r < nranks_; ++r) {
      if (counts[r] == 0) continue;
      const char* src = static_cast<const char*>(sendbuf) + displs[r] * es;
      if (r == root) {
        HIP_THROW(hipMemcpyAsync(recvbuf, src, counts[r] * es, hipMemcpyDeviceToDevice, s));
      } else {
        NCCL_THROW(ncclSend(src, counts[r], dt, r, comm_, s));
      }
    }
  } else if (counts[rank_] > 0) {
    NCCL_THROW(ncclRecv(recvbuf, counts[rank_], dt, root, comm_, s));
  }
  NCCL_THROW(ncclGroupEnd());
}

size_t RcclComm::acc32_slice(size_t count) const {
  const size_t per = (count + nranks_ - 1) / nranks_;
  return (per + 63) / 64 * 64;
}

void RcclComm::allreduce_bf16_acc32(void* buf, void* scratch, size_t count, hipStream_t s) {
  if (nranks_ == 1) return;
  const size_t c = acc32_slice(count);
  auto off = [&](int r) { return std::min(count, (size_t)r * c); };
  auto cnt = [&](int r) { return std::min(count, (size_t)(r + 1) * c) - off(r); };
  bf16* b = static_cast<bf16*>(buf);
  bf16* sc = static_cast<bf16*>(scratch);
  // 1) all-to-all: slice q of my buffer to its owner q; every peer's copy of my slice into
  //    scratch slot [peer]
  NCCL_THROW(ncclGroupStart());
  for (int q = 0; q < nranks_; ++q) {
    if (q == rank_) continue;
    if (cnt(q) > 0) NCCL_THROW(ncclSend(b + off(q), cnt(q), ncclBfloat16, q, comm_, s));
    if (cnt(rank_) > 0) NCCL_THROW(ncclRecv(sc + (size_t)q * c, cnt(rank_), ncclBfloat16, q, comm_, s));
  }
  NCCL_THROW(ncclGroupEnd());
  // 2) the owner's fp32 sum in rank order, one rounding, in place in its slice
  if (cnt(rank_) > 0)
    HIP_THROW(sum_slices_bf16(b + off(rank_), sc, nranks_, rank_, (long long)c,
                              (long long)cnt(rank_), s));
  // 3) all-gather of the reduced slices (grouped send/recv: uneven last slices)
  NCCL_THROW(ncclGroupStart());
  for (int q = 0; q < nranks_; ++q) {
    if (q == rank_) continue;
    if (cnt(rank_) > 0) NCCL_THROW(ncclSend(b + off(rank_), cnt(rank_), ncclBfloat16, q, comm_, s));
    if (cnt(q) > 0) NCCL_THROW(ncclRecv(b + off(q), cnt(q), ncclBfloat16, q, comm_, s));
  }
  NCCL_THROW(ncclGroupEnd());
}

void RcclComm::allreduce_f32_ordered(void* buf, void* scratch, size_t count, hipStream_t s) {
  if (nranks_ == 1) return;
  const size_t c = acc32_slice(count);
  auto off = [&](int r) { return std::min(count, (size_t)r * c); };
  auto cnt = [&](int r) { return std::min(count, (size_t)(r + 1) * c) - off(r); };
  float* b = static_cast<float*>(buf);
  float* sc = static_cast<float*>(scratch);
  NCCL_THROW(ncclGroupStart());
  for (int q = 0; q < nranks_; ++q) {
    if (q == rank_) continue;
    if (cnt(q) > 0) NCCL_THROW(ncclSend(b + off(q), cnt(q), ncclFloat32, q, comm_, s));
    if (cnt(rank_) > 0) NCCL_THROW(ncclRecv(sc + (size_t)q * c, cnt(rank_), ncclFloat32, q, comm_, s));
  }
  NCCL_THROW(ncclGroupEnd());
  if (cnt(rank_) > 0)
    HIP_THROW(sum_slices_f32(b + off(rank_), sc, nranks_, rank_, (long long)c, (long long)cnt(rank_), s));
  NCCL_THROW(ncclGroupStart());
  for (int q = 0; q < nranks_; ++q) {
    if (q == rank_) continue;
    if (cnt(rank_) > 0) NCCL_THROW(ncclSend(b + off(rank_), cnt(rank_), ncclFloat32, q, comm_, s));
    if (cnt(q) > 0) NCCL_THROW(ncclRecv(b + off(q), cnt(q), ncclFloat32, q, comm_, s));
  }
  NCCL_THROW(ncclGroupEnd());
}

// The reduce-scatter leg of ZeRO-1 with the sums of allreduce_f32_ordered: rank r ends with
// slice r of `buf` (nranks slices of `shard` elements) summed over the ranks in rank order, in
// place -- bit for bit what the ordered all-reduce leaves there (ncclReduceScatter's ring sums
// slice r in the order r+1, r+2, ..., r).  scratch: nranks * shard floats.
void RcclComm::reduce_scatter_f32_ordered(void* buf, void* scratch, size_t shard, hipStream_t s) {
  if (nranks_ == 1 || shard == 0) return;
  float* b = static_cast<float*>(buf);
  float* sc = static_cast<float*>(scratch);
  NCCL_THROW(ncclGroupStart());
  for (int q = 0; q < nranks_; ++q) {
    if (q == rank_) continue;
    NCCL_THROW(ncclSend(b + (size_t)q * shard, shard, ncclFloat32, q, comm_, s));
    NCCL_THROW(ncclRecv(sc + (size_t)q * shard, shard, ncclFloat32, q, comm_, s));
  }
  NCCL_THROW(ncclGroupEnd());
  HIP_THROW(sum_slices_f32(b + (size_t)rank_ * shard, sc, nranks_, rank_, (long long)shard,
                           (long long)shard, s));
}

int RcclComm::poll_error(bool abort_on_error) {
  if (aborted_) return (int)ncclInvalidUsage;
  ncclResult_t r = ncclSuccess;
  // the query itself can fail (e.g. a communicator torn down underneath us): that is an error
  // of the communicator too, never "healthy"
  const ncclResult_t q = ncclCommGetAsyncError(comm_, &r);
  if (q != ncclSuccess) r = q;
  if (r != ncclSuccess && r != ncclInProgress && abort_on_error) abort();
  return r == ncclInProgress ? 0 : (int)r;
}

void RcclComm::broadcast_pieces(void* base, const std::vector<long long>& offsets,
                                const std::vector<long long>& counts,
                                const std::vector<int>& roots, int dtype, hipStream_t s) {
  if (offsets.size() != counts.size() || offsets.size() != roots.size())
    throw std::runtime_error("broadcast_pieces: offsets/counts/roots differ in length");
  if (offsets.empty()) return;
  const size_t es = dtype_size(dtype);
  const ncclDataType_t dt = to_nccl(dtype);
  NCCL_THROW(ncclGroupStart());
  for (size_t i = 0; i < offsets.size(); ++i) {
    if (counts[i] <= 0) continue;
    if (roots[i] < 0 || roots[i] >= nranks_) throw std::runtime_error("broadcast_pieces: bad root");
    char* p = static_cast<char*>(base) + offsets[i] * es;
    NCCL_THROW(ncclBroadcast(p, p, counts[i], dt, roots[i], comm_, s));
  }
  NCCL_THROW(ncclGroupEnd());
}

void RcclComm::abort() {
  if (comm_ && !aborted_) {
    ncclCommAbort(comm_);
    aborted_ = true;
  }
}

// ---------------------------------------------------------------------------------------------
GradSync::GradSync(RcclComm* comm, int n_buckets, int priority) : comm_(comm) {
  HIP_THROW(hipStreamCreateWithPriority(&comm_stream_, hipStreamNonBlocking, priority));
  ready_.resize(n_buckets);
  for (auto& e : ready_) HIP_THROW(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIP_THROW(hipEventCreateWithFlags(&done_, hipEventDisableTiming));
}

GradSync::~GradSync() {
  for (auto& e : ready_) (void)hipEventDestroy(e);
  if (done_) (void)hipEventDestroy(done_);
  if (comm_stream_) (void)hipStreamDestroy(comm_stream_);
}

void GradSync::bucket_ready(int b, void* ptr, size_t count, int dtype, hipStream_t compute) {
  if (b < 0 || b >= (int)ready_.size()) throw std::runtime_error("bucket index out of range");
  HIP_THROW(hipEventRecord(ready_[b], compute));
  HIP_THROW(hipStreamWaitEvent(comm_stream_, ready_[b], 0));
  if (dtype == 1 && acc32_scratch_)
    comm_->allreduce_bf16_acc32(ptr, acc32_scratch_, count, comm_stream_);
  else if (dtype == 0 && f32_scratch_)
    comm_->allreduce_f32_ordered(ptr, f32_scratch_, count, comm_stream_);
  else
    comm_->allreduce(ptr, count, dtype, 0, comm_stream_);
  if (standin_blocks_ > 0 && standin_gbps_ > 0.0) {
    // a ring all-reduce moves 2 (P-1)/P of the bytes per rank; at P = 8: 1.75
    const double bytes = 1.75 * (double)count * (dtype == 1 ? 2.0 : 4.0);
    if (!cu_hold) throw std::runtime_error("collective stand-in: experiments build only");
    HIP_THROW(cu_hold(standin_blocks_, bytes / (standin_gbps_ * 1e9), comm_stream_));
  }
}

void GradSync::join(hipStream_t compute) {
  HIP_THROW(hipEventRecord(done_, comm_stream_));
  HIP_THROW(hipStreamWaitEvent(compute, done_, 0));
}

// ---------------------------------------------------------------------------------------------
GraphRunner::~GraphRunner() {
  if (exec_) (void)hipGraphExecDestroy(exec_);
  if (graph_) (void)hipGraphDestroy(graph_);
}

void GraphRunner::begin(hipStream_t s, int mode) {
  if (exec_) { (void)hipGraphExecDestroy(exec_); exec_ = nullptr; }
  if (graph_) { (void)hipGraphDestroy(graph_); graph_ = nullptr; }
  cap_ = s;
  const hipStreamCaptureMode m = mode == 0 ? hipStreamCaptureModeGlobal
                               : mode == 2 ? hipStreamCaptureModeRelaxed
                                           : hipStreamCaptureModeThreadLocal;
  HIP_THROW(hipStreamBeginCapture(s, m));
}

void GraphRunner::end() {
  hipStream_t s = cap_;
  const hipError_t e = hipStreamEndCapture(cap_, &graph_);
  cap_ = nullptr;
  if (e != hipSuccess) {
    if (graph_) { (void)hipGraphDestroy(graph_); graph_ = nullptr; }
    (void)hipGetLastError();
    throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e) +
                             " at hipStreamEndCapture");
  }
  HIP_THROW(hipGraphInstantiate(&exec_, graph_, nullptr, nullptr, 0));
  // Upload the executable graph now (asynchronously on the capture stream), so its first
  // replay -- often inside a timed region -- does not pay for it.  NNMPI_GRAPH_UPLOAD=0 skips
  // it (A/B).
  static const bool upload = [] {
    const char* v = knob_env("NNMPI_GRAPH_UPLOAD");
    return !(v && v[0] == '0');
  }();
  if (upload) HIP_THROW(hipGraphUpload(exec_, s));
}

void GraphRunner::cancel() {
  // A throw while the stream was capturing (a collective refused, a shape check): end the
  // capture and drop the partial graph, so the stream is usable again and no half-captured
  // work is ever replayed.
  if (cap_) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(cap_, &st) == hipSuccess && st != hipStreamCaptureStatusNone) {
      hipGraph_t g = nullptr;
      (void)hipStreamEndCapture(cap_, &g);
      if (g) (void)hipGraphDestroy(g);
    }
    cap_ = nullptr;
  }
  if (exec_) { (void)hipGraphExecDestroy(exec_); exec_ = nullptr; }
  if (graph_) { (void)hipGraphDestroy(graph_); graph_ = nullptr; }
  (void)hipGetLastError();
}

void GraphRunner::launch(hipStream_t s) {
  if (!exec_) throw std::runtime_error("graph not captured");
  HIP_THROW(hipGraphLaunch(exec_, s));
}

size_t GraphRunner::num_nodes() const {
  if (!graph_) return 0;
  size_t n = 0;
  (void)hipGraphGetNodes(graph_, nullptr, &n);
  return n;
}

}  // namespace nnmpi
