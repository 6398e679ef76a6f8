// softmax.hip -- in-batch sampled-softmax loss of tfrs.tasks.Retrieval, forward and
// backward, without materialising the [nq, nc] logits; for 2-D queries q[nq, d] and for
// MULTI-HEAD (max-sim) queries q[nq, H, d], then also without the [nq*H, nc] head scores.
//
// Replaces (tasks/retrieval.py) the scores matmul :178-180 (multi-head: einsum "qne,ce->qnc" and
// reduce_max over heads :172-176), labels=eye :185, temperature
// :187-188, SamplingProbablityCorrection :190-192 (layers/loss.py:150-158),
// RemoveAccidentalHits :194-200 (layers/loss.py:114-147), score_mask :202-203 and the Keras
// CategoricalCrossentropy(from_logits, SUM) :210, plus their gradients
// (models/base.py:77).
//
//   M_bc  = max_h (q_bh . c_c)                 (the max is taken on the raw dot products; H = 1: q_b . c_c)
//   S_bc  = M_bc * inv_t - corr_c  [+ MIN_FLOAT if ids_c == ids_b, c != b]
//           [= MIN_FLOAT where !mask_bc]                                          (make_logit)
//   loss  = sum_b w_b (logsumexp_c S_bc - S_bb)
//   G_bc  = gloss * w_b * (exp(S_bc - lse_b) - [b == c]) * inv_t      (0 where masked)
//   h*(b,c) = the LOWEST head index attaining the max (torch.max(dim) / first-index rule; TensorFlow's
//             reduce_max splits the gradient among tied heads instead)
//   dq_bh = sum_c [h == h*(b,c)] G_bc c_c ,   dc_c = sum_b G_bc q_{b,h*(b,c)}
//
// Structure (flash-attention like): a wave owns 32 rows of one side as the MFMA B operand
// and streams 32-row tiles of the other side as the A operand straight from L2 (both
// embedding matrices of a batch are a few MB).  Lanes index the owned rows, accumulator
// registers index the streamed rows, so the online max/sum of a row is lane-local.  In
// the backward the tile of G stays in the accumulator layout and is fed back as the B
// operand of the second GEMM (out^T[feature][row] += X^T G) -- no transposes.
// The streamed side is split across waves for occupancy; partial (max, sum) pairs and
// partial gradients are combined by small deterministic reduce kernels (no float atomics).
//
// Head layout (MH = true): the rows on the query side are the flat (query, head) rows with a query's
// heads ADJACENT: with Hp = the next power of two >= H a block of 32 rows holds 32 / Hp queries, head
// slot = row & (Hp - 1); slots H .. Hp-1 load zeros and enter the max as -inf.
//   forward, dq : the wave owns such a block, so a query's heads are lanes that differ in the low
//                 log2(Hp) bits of lane & 31: the head max of an accumulator register is log2(Hp)
//                 xor-exchanges, the lowest maximal head is the lowest set bit of the group's field of
//                 one ballot.  Every lane of a head group then carries the same online (m, l); head slot 0
//                 writes it.  dq multiplies G only into the winning head's lane.
//   dc          : the wave owns candidates and streams the flat rows, so a query's heads are accumulator
//                 registers: tile row (r & 3) + 8 (r >> 2) + 4 h.  Hp <= 4: register-local (r ^ 1, r ^ 2);
//                 Hp >= 8 adds one exchange with lane ^ 32, Hp = 16 / 32 the registers r ^ 4 / r ^ 8.
// MH = false is the same kernel at H = Hp = 1 with the head steps compiled out: the 2-D entry points.
//
// The tile loops themselves live in softmax_shared.h (softmax_stream_queries + OnlineSoftmax: the forward;
// softmax_bwd_body: dq and dc) and are shared with the mined kernels of softmax_mined.hip; the kernels here
// instantiate them with the plain policy (make_logit, every column kept).
//
// Roofline: MFMA-bound, 2*nq*nc*d flop forward and 8*nq*nc*d backward (S is recomputed
// once per gradient); at the MovieLens batch (4096 x 4096 x 64) the whole step is a few
// tens of microseconds, i.e. launch-latency territory.
#include "softmax_shared.h"

namespace tfrs {

// PLAIN: no sampling-probability correction, no accidental-hit removal, no score mask (the
// default Retrieval configuration): those branches are compiled out of the tile epilogue.
template <bool PLAIN>
__device__ __forceinline__ SoftmaxArgs plain_args(SoftmaxArgs a) {
  if (PLAIN) {
    a.corr = nullptr;
    a.ids = nullptr;
    a.mask = nullptr;
  }
  return a;
}

template <int DP, bool PLAIN, bool MH>
__global__ void __launch_bounds__(256) softmax_fwd_kernel(const SoftmaxArgs a_in) {
  const SoftmaxArgs a = plain_args<PLAIN>(a_in);
  OnlineSoftmax<PlainPolicy> online;
  softmax_stream_queries<DP, MH, 4>(a, PlainPolicy{a}, online);
}

template <int DP, bool ROWS_ARE_QUERIES, bool PLAIN, bool MH>
__global__ void __launch_bounds__(256) softmax_bwd_kernel(const SoftmaxArgs a_in) {
  extern __shared__ __attribute__((aligned(16))) float smem_sm[];
  const SoftmaxArgs a = plain_args<PLAIN>(a_in);
  softmax_bwd_body<DP, ROWS_ARE_QUERIES, MH>(a, PlainPolicy{a}, smem_sm);
}

template <int DP, bool MH>
static void launch_fwd(const SoftmaxArgs &a, hipStream_t s) {
  const int qw = 32 >> a.lhp;
  const int64_t waves = ((a.nq + qw - 1) / qw) * a.nsplit;
  const bool plain = !a.corr && !a.ids && !a.mask;
  hipLaunchKernelGGL((plain ? softmax_fwd_kernel<DP, true, MH> : softmax_fwd_kernel<DP, false, MH>),
                     dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, a);
}

template <int DP, bool RQ, bool MH>
static void launch_bwd(const SoftmaxArgs &a, hipStream_t s) {
  const int qw = 32 >> a.lhp;
  const int64_t blocks = RQ ? (a.nq + qw - 1) / qw : (a.nc + 31) / 32;
  const int64_t waves = blocks * a.nsplit;
  const size_t lds = (size_t)4 * 32 * (DP + 4) * sizeof(float);
  const bool plain = !a.corr && !a.ids && !a.mask;
  hipLaunchKernelGGL((plain ? softmax_bwd_kernel<DP, RQ, true, MH> : softmax_bwd_kernel<DP, RQ, false, MH>),
                     dim3((unsigned)((waves + 3) / 4)), dim3(256), lds, s, a);
}

// workspace of the f32 kernels: the forward's partials or the backward's two partial-gradient buffers
static size_t f32_workspace_bytes(int64_t nq, int heads, int64_t nc, int d) {
  const SoftmaxLayout L = softmax_layout(nq, heads, nc, d);
  return std::max(L.fwd, L.bwd);
}

template <bool MH>
static int run_fwd(SoftmaxArgs a, float *out_loss, float *out_lse, float *out_pos, void *workspace, hipStream_t s) {
  return softmax_run_fwd(a, out_loss, out_lse, out_pos, workspace, s,
                         [&](auto dp) { launch_fwd<decltype(dp)::value, MH>(a, s); });
}

template <bool MH>
static int run_bwd(SoftmaxArgs a, float *dq, float *dc, void *workspace, hipStream_t s) {
  return softmax_run_bwd(a, dq, dc, workspace, s,
                         [&](auto dp, auto rq) { launch_bwd<decltype(dp)::value, decltype(rq)::value, MH>(a, s); });
}

// softmax16.hip: the split-fp16 path
size_t softmax16_workspace_bytes(int64_t nq, int64_t nc, int d);
int softmax16_forward(const float *q, const float *c, int64_t nq, int64_t nc, int d, const float *w,
                      float inv_t, float *out_loss, float *out_lse, float *out_pos, void *ws,
                      hipStream_t s);
int softmax16_backward(const float *q, const float *c, int64_t nq, int64_t nc, int d, const float *w,
                       float inv_t, const float *lse, const float *gloss, float *dq, float *dc,
                       void *ws, int reuse, hipStream_t s);

// TFRS_SOFTMAX_MODE=f32 keeps everything on the f32-MFMA kernels; default: the split-fp16 path
// whenever no logit option that needs per-element side inputs is set.
static bool use_f16_path(const float *corr, const int64_t *ids, const uint8_t *mask) {
  const char *v = option("TFRS_SOFTMAX_MODE");   // read per call: tests switch it
  const bool f32_only = v && v[0] == 'f' && v[1] == '3';
  return !f32_only && !corr && !ids && !mask;
}

}  // namespace tfrs

using namespace tfrs;

// ---- 2-D queries: the MH = false kernels, or the split-fp16 path
static int check_common(const float *q, const float *c, int64_t nq, int64_t nc, int d,
                        const char *who) {
  TFRS_CHECK_ARG(nq >= 1 && nc >= 1 && d >= 1, "%s: bad shape", who);
  TFRS_CHECK_ARG(nc >= nq, "%s: needs num_candidates >= num_queries (labels = eye)", who);
  TFRS_CHECK_ARG(q && c, "%s: NULL pointer", who);
  if (d > 128) {
    set_error("%s: embedding dim %d > 128 is not implemented", who, d);
    return TFRS_ENOTIMPL;
  }
  return TFRS_OK;
}

extern "C" size_t tfrs_inbatch_softmax_workspace_bytes(int64_t nq, int64_t nc, int d) {
  if (nq < 1 || nc < 1 || d < 1) return 256;
  const size_t f32 = f32_workspace_bytes(nq, 1, nc, d);
  const size_t f16 = d <= 128 ? softmax16_workspace_bytes(nq, nc, d) : 0;
  return f32 > f16 ? f32 : f16;
}

extern "C" int tfrs_inbatch_softmax_ce_fwd(const float *q, const float *c, int64_t nq, int64_t nc,
                                           int d, const float *sample_weight,
                                           float inv_temperature, const float *log_q_correction,
                                           const int64_t *cand_ids, const uint8_t *score_mask,
                                           float *out_loss, float *out_lse, float *out_pos,
                                           void *workspace, size_t workspace_bytes, void *stream) {
  int rc = check_common(q, c, nq, nc, d, "inbatch_softmax_ce_fwd");
  if (rc != TFRS_OK) return rc;
  TFRS_CHECK_ARG(out_loss && out_lse && out_pos && workspace, "inbatch_softmax_ce_fwd: NULL output");
  if (workspace_bytes < tfrs_inbatch_softmax_workspace_bytes(nq, nc, d)) {
    set_error("inbatch_softmax_ce_fwd: workspace too small");
    return TFRS_ENOMEM;
  }
  if (use_f16_path(log_q_correction, cand_ids, score_mask))
    return softmax16_forward(q, c, nq, nc, d, sample_weight, inv_temperature, out_loss, out_lse,
                             out_pos, workspace, (hipStream_t)stream);
  return run_fwd<false>(softmax_args(q, c, nq, 1, nc, d, sample_weight, inv_temperature, log_q_correction,
                                  cand_ids, score_mask),
                        out_loss, out_lse, out_pos, workspace, (hipStream_t)stream);
}

extern "C" int tfrs_inbatch_softmax_ce_bwd(const float *q, const float *c, int64_t nq, int64_t nc,
                                           int d, const float *sample_weight,
                                           float inv_temperature, const float *log_q_correction,
                                           const int64_t *cand_ids, const uint8_t *score_mask,
                                           const float *lse, const float *gloss, float *dq,
                                           float *dc, void *workspace, size_t workspace_bytes,
                                           int reuse_forward_workspace, void *stream) {
  int rc = check_common(q, c, nq, nc, d, "inbatch_softmax_ce_bwd");
  if (rc != TFRS_OK) return rc;
  TFRS_CHECK_ARG(lse && dq && dc && workspace, "inbatch_softmax_ce_bwd: NULL pointer");
  if (workspace_bytes < tfrs_inbatch_softmax_workspace_bytes(nq, nc, d)) {
    set_error("inbatch_softmax_ce_bwd: workspace too small");
    return TFRS_ENOMEM;
  }
  if (use_f16_path(log_q_correction, cand_ids, score_mask))
    return softmax16_backward(q, c, nq, nc, d, sample_weight, inv_temperature, lse, gloss, dq, dc,
                              workspace, reuse_forward_workspace, (hipStream_t)stream);
  SoftmaxArgs a = softmax_args(q, c, nq, 1, nc, d, sample_weight, inv_temperature, log_q_correction, cand_ids,
                            score_mask);
  a.lse = lse; a.gloss = gloss;
  return run_bwd<false>(a, dq, dc, workspace, (hipStream_t)stream);
}

// The split geometry of the f32 kernels under the options in force (host only, no device call): nsplit and split_len
// of the forward / dq kernels and of the dc kernel, from the layout the launches above use.
extern "C" int tfrs_inbatch_softmax_plan_f32(int64_t nq, int heads, int64_t nc, int64_t *out) {
  TFRS_CHECK_ARG(nq >= 1 && nc >= nq && heads >= 1 && heads <= 32 && out, "inbatch_softmax_plan_f32: bad argument");
  const SoftmaxLayout L = softmax_layout(nq, heads, nc, 1);
  out[0] = L.nsq; out[1] = L.lenq; out[2] = L.nsc; out[3] = L.lenc;
  return TFRS_OK;
}

// ---- multi-head queries: the MH = true kernels for every heads in 1 .. 32
static int check_common_mh(const float *q, const float *c, int64_t nq, int heads, int64_t nc, int d,
                           const char *who) {
  TFRS_CHECK_ARG(nq >= 1 && nc >= 1, "%s: bad shape (nq=%lld, nc=%lld)", who, (long long)nq, (long long)nc);
  TFRS_CHECK_ARG(heads >= 1 && heads <= 32, "%s: heads=%d outside [1, 32]", who, heads);
  TFRS_CHECK_ARG(d >= 1 && d <= TFRS_MAX_DIM, "%s: embedding dim=%d outside [1, %d]", who, d, TFRS_MAX_DIM);
  TFRS_CHECK_ARG(nc >= nq, "%s: needs num_candidates >= num_queries (labels = eye)", who);
  TFRS_CHECK_ARG(q && c, "%s: NULL pointer", who);
  return TFRS_OK;
}

extern "C" size_t tfrs_inbatch_softmax_mh_workspace_bytes(int64_t nq, int heads, int64_t nc, int d) {
  if (nq < 1 || nc < 1 || d < 1 || heads < 1 || heads > 32) return 256;
  return f32_workspace_bytes(nq, heads, nc, d);
}

extern "C" int tfrs_inbatch_softmax_mh_ce_fwd(const float *q, const float *c, int64_t nq, int heads, int64_t nc,
                                              int d, const float *sample_weight, float inv_temperature,
                                              const float *log_q_correction, const int64_t *cand_ids,
                                              const uint8_t *score_mask, float *out_loss, float *out_lse,
                                              float *out_pos, void *workspace, size_t workspace_bytes,
                                              void *stream) {
  int rc = check_common_mh(q, c, nq, heads, nc, d, "inbatch_softmax_mh_ce_fwd");
  if (rc != TFRS_OK) return rc;
  TFRS_CHECK_ARG(out_loss && out_lse && out_pos && workspace, "inbatch_softmax_mh_ce_fwd: NULL output");
  TFRS_CHECK_ARG(workspace_bytes >= tfrs_inbatch_softmax_mh_workspace_bytes(nq, heads, nc, d),
                 "inbatch_softmax_mh_ce_fwd: workspace too small");
  return run_fwd<true>(softmax_args(q, c, nq, heads, nc, d, sample_weight, inv_temperature, log_q_correction,
                                 cand_ids, score_mask),
                       out_loss, out_lse, out_pos, workspace, (hipStream_t)stream);
}

extern "C" int tfrs_inbatch_softmax_mh_ce_bwd(const float *q, const float *c, int64_t nq, int heads, int64_t nc,
                                              int d, const float *sample_weight, float inv_temperature,
                                              const float *log_q_correction, const int64_t *cand_ids,
                                              const uint8_t *score_mask, const float *lse, const float *gloss,
                                              float *dq, float *dc, void *workspace, size_t workspace_bytes,
                                              void *stream) {
  int rc = check_common_mh(q, c, nq, heads, nc, d, "inbatch_softmax_mh_ce_bwd");
  if (rc != TFRS_OK) return rc;
  TFRS_CHECK_ARG(lse && dq && dc && workspace, "inbatch_softmax_mh_ce_bwd: NULL pointer");
  TFRS_CHECK_ARG(workspace_bytes >= tfrs_inbatch_softmax_mh_workspace_bytes(nq, heads, nc, d),
                 "inbatch_softmax_mh_ce_bwd: workspace too small");
  SoftmaxArgs a = softmax_args(q, c, nq, heads, nc, d, sample_weight, inv_temperature, log_q_correction, cand_ids,
                            score_mask);
  a.lse = lse; a.gloss = gloss;
  return run_bwd<true>(a, dq, dc, workspace, (hipStream_t)stream);
}
