// The plain supervised multi-task head loss as ONE device op: value, log record and the gradient with respect to every task's
// box / cls / dir head outputs, all tasks in the same launches, nothing read back -- so it can sit inside a captured iteration.
// This is the loss of the reference's three-class SECOND config and of its PointPillars config (not the SE-SSD one of
// head_loss.hip: no teacher, no ODIoU, no IoU prediction; the smooth-L1 localisation term is the real regression loss here).
//
// Replaces, per task:
//   det3d/models/bbox_heads/mg_head.py:559-652   MultiGroupHead.loss
//   det3d/models/bbox_heads/mg_head.py:155-193   create_loss, :34-39 add_sin_difference, :42-54 _get_pos_neg_loss,
//                                                :57-71 get_direction_target, :535-538 prepare_loss_weights (NormByNumPositives)
//   det3d/models/losses/losses.py:146-203 (WeightedSmoothL1Loss), :364-418 (SigmoidFocalLoss), :489-531 (softmax CE)
//   the trainer's sum over the tasks' `loss` entries (parse_second_losses)
// The torch formulation is some sixty small ops per task, with reductions that do not survive a replayed hipGraph.
//
// Launches (one stream, task on grid axis z, sample on y, 256-anchor block on x):
//   1 sl_count   positives (label > 0) of every block
//   2 sl_anchor  positives of the block's sample (from launch 1) -> focal term + gradient for every anchor; in a block WITH
//                positives also the box / target slabs (256 x 7 floats, staged through LDS: global reads and writes are
//                lane-contiguous, the per-anchor reads are at stride 7 words = conflict free), smooth-L1 and direction terms on
//                the positives with their gradients; a block without positives reads neither slab and writes zeros.
//                Twelve block partials in double.
//   3 sl_final   ordered sums of the partials -> one record row per task and the row of the tasks' sum
// Summation order is fixed (terms in double, waves and blocks in index order): deterministic, no float atomics.
#include "common.hpp"
#include "sessd_hip_types.h"

namespace {

constexpr int NT = 256;
constexpr int NPART = 12;   // cls, cls over positives, cls over negatives, dir, loc[7], number of negatives
constexpr int REC = 32;     // floats of one record row
constexpr int MAXT = 4;

struct Tasks {
  sessd_supervised_task_t t[MAXT];
};

struct Work {
  int* blk_cnt;   // [T][B][nblk] positives of a block
  int* counts;    // [T][B]       positives of a sample
  double* part;   // [T][B][nblk][NPART]
};

__device__ __forceinline__ int load_label(const void* labels, int i64, size_t i) {
  return i64 ? (int)((const long long*)labels)[i] : ((const int*)labels)[i];
}

// WeightedSmoothL1Loss element (losses.py:188-193), sigma^2 = s2: value and derivative with respect to diff (0 at diff == 0)
__device__ __forceinline__ float sl1(float diff, float s2, float* d) {
  const float a = fabsf(diff);
  if (a <= 1.0f / s2) {
    *d = s2 * diff;
    const float t = a * sqrtf(s2);
    return 0.5f * (t * t);
  }
  *d = diff > 0.f ? 1.0f : (diff < 0.f ? -1.0f : 0.0f);
  return a - 0.5f / s2;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over the block's NT threads, valid in every thread; `sm` holds NT / 64 ints
__device__ __forceinline__ int block_sum_i(int v, int* sm) {
  v = sessd_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) t += sm[w];
  return t;
}

// ---------------------------------------------------------------------------------------------------------------- launch 1
__global__ __launch_bounds__(NT) void sl_count_kernel(Tasks TK, sessd_supervised_loss_cfg_t P, Work W, int nblk) {
  __shared__ int sm[NT / 64];
  const int t = blockIdx.z, b = blockIdx.y, blk = blockIdx.x;
  const int a = blk * NT + threadIdx.x;
  int pos = 0;
  if (a < P.num_anchors) pos = load_label(TK.t[t].labels, P.labels_i64, (size_t)b * P.num_anchors + a) > 0;
  const int npos = block_sum_i(pos, sm);
  if (threadIdx.x == 0) W.blk_cnt[((size_t)t * P.batch + b) * nblk + blk] = npos;
}

// ---------------------------------------------------------------------------------------------------------------- launch 2
__global__ __launch_bounds__(NT) void sl_anchor_kernel(Tasks TK, sessd_supervised_loss_cfg_t P, Work W, int nblk) {
  __shared__ int smi[NT / 64];
  __shared__ double smd[NT / 64][NPART];
  __shared__ float s_box[NT * 7];   // box codes in, box gradients out
  __shared__ float s_tg[NT * 7];    // regression targets
  const int t = blockIdx.z, b = blockIdx.y, blk = blockIdx.x, B = P.batch, A = P.num_anchors, tid = threadIdx.x;
  const sessd_supervised_task_t& K = TK.t[t];
  // ---- positives of this sample, of this block: from the per-block counts of launch 1 (nblk ints, ~2 per thread)
  const int* cnt = W.blk_cnt + ((size_t)t * B + b) * nblk;
  int pos_sample = 0;
  for (int i = tid; i < nblk; i += NT) pos_sample += cnt[i];
  pos_sample = block_sum_i(pos_sample, smi);
  const bool any_pos = cnt[blk] > 0;   // the same in every thread of the block
  if (tid == 0 && blk == 0) W.counts[t * B + b] = pos_sample;
  const float norm = fmaxf((float)pos_sample, 1.0f);   // NormByNumPositives (mg_head.py:535-538)
  const int n = min(NT, A - blk * NT);                 // live anchors of this block
  const size_t i0 = (size_t)b * A + (size_t)blk * NT;  // its first anchor
  const bool live = tid < n;
  const size_t i = i0 + (live ? tid : 0);
  if (any_pos) {
    const float* gb = K.box + i0 * 7;
    const float* gt = K.reg_targets + i0 * 7;
    for (int j = tid; j < n * 7; j += NT) {
      s_box[j] = gb[j];
      s_tg[j] = gt[j];
    }
    __syncthreads();
  }
  double part[NPART];
#pragma unroll
  for (int k = 0; k < NPART; ++k) part[k] = 0.0;
  if (live) {
    const int label = load_label(K.labels, P.labels_i64, i);
    const bool pos = label > 0, neg = label == 0;
    // ---- focal classification loss (losses.py:364-418), one class: target 1 on the positives, 0 elsewhere (mg_head.py:586)
    const float x = K.cls[i];
    const float cls_w = ((neg ? P.neg_cls_weight : 0.f) + (pos ? P.pos_cls_weight : 0.f)) / norm;
    const float p = 1.0f / (1.0f + expf(-x)), q = 1.0f / (1.0f + expf(x));   // sigmoid(x), 1 - sigmoid(x) without cancellation
    const float ce = fmaxf(x, 0.f) - (pos ? x : 0.f) + log1pf(expf(-fabsf(x)));
    const float base = pos ? q : p;   // 1 - p_t
    const float g = P.focal_gamma;
    const float mod = g == 2.0f ? base * base : (g == 0.f ? 1.0f : powf(base, g));
    const float dmod = g == 2.0f ? 2.f * base : ((g == 0.f || !(base > 0.f)) ? 0.f : g * powf(base, g - 1.f));
    const float aw = pos ? P.focal_alpha : 1.f - P.focal_alpha;
    const float fl = mod * aw * ce * cls_w;
    const float dbase = pos ? -(p * q) : p * q;
    K.grad_cls[i] = cls_w * aw * (dmod * dbase * ce + mod * (pos ? -q : p)) * (P.cls_loss_weight / (float)B);
    part[0] = fl;
    part[1] = pos ? fl : 0.f;
    part[2] = neg ? fl : 0.f;
    part[11] = neg ? 1.0 : 0.0;
    float gd0 = 0.f, gd1 = 0.f;
    if (any_pos) {
      float* sb = s_box + tid * 7;
      if (pos) {
        const float reg_w = 1.0f / norm;
        const float* st = s_tg + tid * 7;
        // ---- direction classifier (mg_head.py:57-71,618-626; softmax cross entropy losses.py:489-531)
        const float an_r = K.anchors[i * 7 + 6];
        const int dt = ((st[6] + an_r) - P.direction_offset) > 0.f ? 1 : 0;
        const float2 l = *(const float2*)(K.dir + i * 2);
        const float m = fmaxf(l.x, l.y);
        const float e0 = expf(l.x - m), e1 = expf(l.y - m);
        const float lse = m + logf(e0 + e1);
        part[3] = (lse - (dt ? l.y : l.x)) * reg_w;
        const float sd = reg_w * P.dir_loss_weight / (float)B;
        gd0 = (e0 / (e0 + e1) - (dt ? 0.f : 1.f)) * sd;
        gd1 = (e1 / (e0 + e1) - (dt ? 1.f : 0.f)) * sd;
        // ---- smooth-L1 localisation on the sin-encoded yaw (mg_head.py:34-39,187-191)
        const float s2 = P.smooth_l1_sigma * P.smooth_l1_sigma;
        const float sl = reg_w * P.loc_loss_weight / (float)B;
        float d;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          part[4 + k] = sl1(sb[k] - st[k], s2, &d) * reg_w;
          sb[k] = d * sl;
        }
        const float sp = sinf(sb[6]), cp = cosf(sb[6]), sg = sinf(st[6]), cg = cosf(st[6]);
        part[10] = sl1(sp * cg - cp * sg, s2, &d) * reg_w;
        sb[6] = d * (cp * cg + sp * sg) * sl;
      } else {
#pragma unroll
        for (int k = 0; k < 7; ++k) sb[k] = 0.f;
      }
    }
    *(float2*)(K.grad_dir + i * 2) = make_float2(gd0, gd1);
  }
  // ---- the box gradients of the block, lane-contiguous
  {
    float* gg = K.grad_box + i0 * 7;
    if (any_pos) {
      __syncthreads();
      for (int j = tid; j < n * 7; j += NT) gg[j] = s_box[j];
    } else {
      for (int j = tid; j < n * 7; j += NT) gg[j] = 0.f;
    }
  }
  // ---- block partials: waves in index order (a block without positives has only the three focal sums)
  const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int k = 0; k < NPART; ++k) {
    if (!any_pos && (k == 1 || (k >= 3 && k <= 10))) continue;
    const double v = wave_sum_d(part[k]);
    if (lane == 0) smd[wv][k] = v;
  }
  __syncthreads();
  if (tid < NPART) {
    double v = 0.0;
    if (any_pos || !(tid == 1 || (tid >= 3 && tid <= 10)))
      for (int w = 0; w < NT / 64; ++w) v += smd[w][tid];
    W.part[(((size_t)t * B + b) * nblk + blk) * NPART + tid] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------- launch 3
__global__ __launch_bounds__(NT) void sl_final_kernel(sessd_supervised_loss_cfg_t P, Work W, int nblk, float* __restrict__ record) {
  __shared__ double smd[NT / 64][NPART];
  __shared__ double tot[MAXT][NPART];
  const int B = P.batch, T = P.num_tasks, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int t = 0; t < T; ++t) {
    double acc[NPART];
#pragma unroll
    for (int k = 0; k < NPART; ++k) acc[k] = 0.0;
    // per-thread strided, then a fixed tree: the order depends on (B, nblk) only
    for (int i = tid; i < B * nblk; i += NT) {
      const double* p = W.part + ((size_t)t * B * nblk + i) * NPART;
#pragma unroll
      for (int k = 0; k < NPART - 1; ++k) acc[k] += p[k];
      if (i < nblk) acc[NPART - 1] += p[NPART - 1];   // negatives of sample 0 only (num_neg, mg_head.py:641)
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NPART; ++k) {
      const double v = wave_sum_d(acc[k]);
      if (lane == 0) smd[wv][k] = v;
    }
    __syncthreads();
    if (tid < NPART) {
      double v = 0.0;
      for (int w = 0; w < NT / 64; ++w) v += smd[w][tid];
      tot[t][tid] = v;
    }
  }
  __syncthreads();
  for (int k = tid; k < (T + 1) * REC; k += NT) record[k] = 0.f;
  __syncthreads();
  if (tid != 0) return;
  const double invB = 1.0 / (double)B;
  double sum = 0.0;
  for (int t = 0; t < T; ++t) {
    const double* s = tot[t];
    double loc = 0.0;
    for (int k = 0; k < 7; ++k) loc += s[4 + k];
    const double cls_red = P.cls_loss_weight * s[0] * invB, loc_red = P.loc_loss_weight * loc * invB, dir = s[3] * invB;
    const double loss = loc_red + cls_red + P.dir_loss_weight * dir;   // mg_head.py:616,626
    float* r = record + t * REC;
    r[0] = (float)loss;
    r[1] = (float)cls_red;
    r[2] = (float)loc_red;
    r[3] = (float)dir;                                  // unweighted, as mg_head.py:625,636 logs it
    r[4] = (float)(s[1] * invB / P.pos_cls_weight);
    r[5] = (float)(s[2] * invB / P.neg_cls_weight);
    for (int k = 0; k < 7; ++k) r[6 + k] = (float)(s[4 + k] * invB);
    r[13] = (float)W.counts[t * B];                     // positives of sample 0
    r[14] = (float)s[NPART - 1];                        // negatives of sample 0
    int all = 0;
    for (int b = 0; b < B; ++b) all += W.counts[t * B + b];
    r[15] = (float)all;                                 // positives of the batch
    sum += loss;
  }
  record[T * REC] = (float)sum;
}

size_t carve(char*& p, size_t bytes) {
  const size_t o = (size_t)p;
  p += sessd_align(bytes, 256);
  return o;
}

bool cfg_ok(const sessd_supervised_loss_cfg_t* c) {
  return c && c->batch >= 1 && c->batch <= 1024 && c->num_anchors >= 1 && c->num_tasks >= 1 && c->num_tasks <= MAXT &&
         (long long)c->batch * c->num_anchors < (1ll << 31) && c->smooth_l1_sigma > 0.f && c->pos_cls_weight > 0.f &&
         c->neg_cls_weight > 0.f;
}

Work layout(const sessd_supervised_loss_cfg_t* c, void* base, size_t* total) {
  const size_t T = c->num_tasks, B = c->batch, nblk = sessd_divup(c->num_anchors, NT);
  char* p = (char*)base;
  Work W;
  W.blk_cnt = (int*)carve(p, T * B * nblk * 4);
  W.counts = (int*)carve(p, T * B * 4);
  W.part = (double*)carve(p, T * B * nblk * NPART * 8);
  *total = (size_t)(p - (char*)base);
  return W;
}

}  // namespace

extern "C" {

size_t sessd_supervised_loss_workspace_bytes(const sessd_supervised_loss_cfg_t* cfg) {
  if (!cfg_ok(cfg)) return 0;
  size_t total;
  layout(cfg, nullptr, &total);
  return total;
}

int sessd_supervised_loss(const sessd_supervised_loss_cfg_t* cfg, const sessd_supervised_task_t* tasks, float* record, void* workspace,
                          size_t workspace_bytes, hipStream_t stream) {
  if (!cfg_ok(cfg) || !tasks || !record || !workspace) return SESSD_EINVAL;
  Tasks TK = {};
  for (int t = 0; t < cfg->num_tasks; ++t) {
    const sessd_supervised_task_t& k = tasks[t];
    if (!k.box || !k.cls || !k.dir || !k.labels || !k.reg_targets || !k.anchors || !k.grad_box || !k.grad_cls || !k.grad_dir)
      return SESSD_EINVAL;
    TK.t[t] = k;
  }
  if (((size_t)workspace & 255) != 0) return SESSD_EINVAL;
  size_t need;
  const Work W = layout(cfg, workspace, &need);
  if (workspace_bytes < need) return SESSD_EWORKSPACE;
  const sessd_supervised_loss_cfg_t P = *cfg;
  const int nblk = sessd_divup(P.num_anchors, NT);
  const dim3 grid(nblk, P.batch, P.num_tasks);
  SESSD_LAUNCH(sl_count_kernel, grid, dim3(NT), 0, stream, TK, P, W, nblk);
  SESSD_CHECK_LAUNCH();
  SESSD_LAUNCH(sl_anchor_kernel, grid, dim3(NT), 0, stream, TK, P, W, nblk);
  SESSD_CHECK_LAUNCH();
  SESSD_LAUNCH(sl_final_kernel, dim3(1), dim3(NT), 0, stream, P, W, nblk, record);
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}

}  // extern "C"
