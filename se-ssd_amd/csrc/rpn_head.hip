// Tail of the SECOND-style RPN neck fused with the 1x1 heads of the detection head, on gfx950.
// Replaces, for the neck of the three-class config (one block, one stride-1 up-sampler),
//   det3d/models/necks/rpn_v1.py:60-71,113 (ConvTranspose2d(128, 128, 1, stride=1) + BatchNorm2d + ReLU) and the four 1x1 convs
//   of every task of det3d/models/bbox_heads/mg_head_sessd.py:202-230, 477-481 (Head.forward per task).
// It is the counterpart of ssfa_fuse_head_kernel (dense_conv.hip) for a neck that ends in ONE map instead of a softmax blend.
//
// Workgroup = 64 pixels of one frame, 256 threads = 4 waves.
// Stage 1 (up-sampler, 16 k MACs per pixel) on the exact-f32 matrix cores (v_mfma_f32_32x32x2_f32):
//     U[co][pixel] = relu(scale[co] * sum_ci W[ci][co] * X[ci][pixel] + shift[co])
//   A k = 1 stride-1 transposed conv is a 1x1 conv with the weight transposed: the ConvTranspose2d weight (cin, cout) as it is
//   stored IS the MFMA A operand -- lane (i, h) = (lane & 31, lane >> 5) reads W[2 kp + h][m0 + i], two 128-byte rows per wave.
//   B operand: lane (j, h) reads X[2 kp + h][p0 + j], 32 consecutive pixels of one channel plane; a pixel beyond the map has an
//   out-of-range buffer offset and reads 0. Wave w owns couts 32 w .. 32 w + 31 and both 32-pixel halves (A shared by two MFMAs).
//   Operands go L2 -> VGPR directly, eight k-steps (24 loads) ahead of their use. D (row = (r & 3) + 8 (r >> 2) + 4 h, column =
//   lane & 31) gets the folded BatchNorm and the ReLU and goes to LDS as [channel][pixel] (32 KB): a wave's ds_write_b32 covers 32
//   consecutive pixels per 32-lane half -- conflict-free under the 32-bank rule of ds_write_b32 / ds_read_b32.
// Stage 2 (heads) as ssfa_fuse_head_kernel<22, 32, MULTI> runs it: thread = (pixel, channel quarter) reads its 32 values of U
//   from LDS once (a wave reads 64 consecutive pixels of a channel: conflict-free), then the tasks run one after the other through
//   ONE 22-channel staging of weights (11 KB, all lanes read the same address: broadcast) and quarter sums (22 KB), summed in
//   quarter order, + bias; the score filter of predict runs on the logits while they are at hand, same key encoding.
// U never goes to memory (18 MB written + 18 MB read per 200 x 176 frame in the two-launch form) unless `out` asks for it.
// LDS: 32768 + 11264 + 22528 = 66560 bytes per workgroup, two workgroups per CU (133 KB of the 160 KB).
#include "common.hpp"
#include "sessd_hip_types.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

typedef __amdgpu_buffer_rsrc_t rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float bufload(rsrc_t rsrc, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)voff, (int)soff, 0));
}
#define SESSD_OOB 0x80000000u  // a lane offset beyond any buffer: loads return 0, stores are dropped

template <int NOUT>
__global__ __launch_bounds__(256, 2) void rpn_up_head_kernel(const float* __restrict__ x, const float* __restrict__ up_w,
                                                           const float* __restrict__ up_scale, const float* __restrict__ up_shift,
                                                           int npix, float* __restrict__ out, const float* __restrict__ hw,
                                                           const float* __restrict__ hb, float* __restrict__ hout,
                                                           float score_thresh, unsigned long long* __restrict__ keys, int key_cap,
                                                           int* __restrict__ key_count, int ntask) {
  constexpr int C = 128, CPER = 32, KG = 8;              // channels in and out; channels per quarter; k-steps per register set
  __shared__ float s_u[C * 64];                                   // up-sampler output [channel][pixel]
  __shared__ __attribute__((aligned(16))) float s_hw[NOUT * C];  // head weights (of one task at a time)
  __shared__ float s_acc[4 * NOUT * 64];                          // quarter sums of the head channels
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int j = lane & 31, h = lane >> 5;
  const int b = blockIdx.y, p_base = blockIdx.x * 64;
  const unsigned plane4 = (unsigned)npix * 4u, mbytes = (unsigned)C * plane4;
  const size_t boff = (size_t)b * C * npix;
  const rsrc_t xr = make_rsrc(x + boff, mbytes);
  const rsrc_t wr = make_rsrc(up_w, (unsigned)(C * C) * 4u);
  const rsrc_t ro = make_rsrc(out ? out + boff : x, out ? mbytes : 0u);
  for (int k = threadIdx.x; k < NOUT * C; k += 256) s_hw[k] = hw[k];

  // ---- stage 1: the up-sampler on the matrix cores
  unsigned xo[2], po[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int p = p_base + q * 32 + j;
    po[q] = p < npix ? (unsigned)p * 4u : SESSD_OOB;
    xo[q] = p < npix ? (unsigned)h * plane4 + (unsigned)p * 4u : SESSD_OOB;
  }
  const unsigned wo = (unsigned)((h * C + 32 * wave + j) * 4);
  const unsigned wstep = 2u * C * 4u, xstep = 2u * plane4;  // bytes per k-step (one cin pair)
  f32x16 acc[2];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
  float wa[2][KG], xb[2][KG][2];
#define SESSD_LOAD(SET, G)                                                       \
  {                                                                              \
    _Pragma("unroll") for (int s = 0; s < KG; ++s) {                             \
      const unsigned kp = (unsigned)((G) * KG + s);                              \
      wa[SET][s] = bufload(wr, wo, kp * wstep);                                  \
      xb[SET][s][0] = bufload(xr, xo[0], kp * xstep);                            \
      xb[SET][s][1] = bufload(xr, xo[1], kp * xstep);                            \
    }                                                                            \
  }
#define SESSD_MMA(SET)                                                           \
  {                                                                              \
    _Pragma("unroll") for (int s = 0; s < KG; ++s) {                             \
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[SET][s], xb[SET][s][0], acc[0], 0, 0, 0); \
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[SET][s], xb[SET][s][1], acc[1], 0, 0, 0); \
    }                                                                            \
  }
  // two register sets, every load unconditional (the last one is clamped and unused), issue-next-then-consume in program order
  constexpr int NG = (C / 2) / KG;  // 8 groups of 8 k-steps
  SESSD_LOAD(0, 0)
#pragma unroll
  for (int g = 0; g < NG; g += 2) {
    SESSD_LOAD(1, g + 1)
    __builtin_amdgcn_sched_barrier(0);
    SESSD_MMA(0)
    __builtin_amdgcn_sched_barrier(0);
    SESSD_LOAD(0, (g + 2 < NG ? g + 2 : NG - 1))
    __builtin_amdgcn_sched_barrier(0);
    SESSD_MMA(1)
    __builtin_amdgcn_sched_barrier(0);
  }
#undef SESSD_LOAD
#undef SESSD_MMA
  {
    const int co0 = 32 * wave + 4 * h;
    float scv[16], shv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = (r & 3) + 8 * (r >> 2);
      scv[r] = up_scale[co0 + k];
      shv[r] = up_shift[co0 + k];
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + (r & 3) + 8 * (r >> 2);
        const float u = fmaxf(fmaf(acc[q][r], scv[r], shv[r]), 0.f);
        s_u[co * 64 + q * 32 + j] = u;
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, u), ro, (int)po[q], (int)((unsigned)co * plane4), 0);
      }
  }
  __syncthreads();

  // ---- stage 2: the heads, task by task (thread = pixel x channel quarter)
  const int px = lane, cq = wave;
  const int p = p_base + px;
  const int c0 = cq * CPER;
  const bool live = p < npix;
  float v0[CPER];
#pragma unroll
  for (int c = 0; c < CPER; ++c) v0[c] = s_u[(c0 + c) * 64 + px];
#pragma unroll 1
  for (int t = 0; t < ntask; ++t) {
    if (t > 0) {  // every thread is done with the previous task's weights and quarter sums
      __syncthreads();
      for (int k = threadIdx.x; k < NOUT * C; k += 256) s_hw[k] = hw[(size_t)t * NOUT * C + k];
      __syncthreads();
    }
    float a[NOUT];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) a[o] = 0.f;
#pragma unroll
    for (int c = 0; c < CPER; c += 4) {
#pragma unroll
      for (int o = 0; o < NOUT; ++o) {
        const float4 w = *reinterpret_cast<const float4*>(s_hw + o * C + c0 + c);
        a[o] = fmaf(v0[c + 0], w.x, a[o]);
        a[o] = fmaf(v0[c + 1], w.y, a[o]);
        a[o] = fmaf(v0[c + 2], w.z, a[o]);
        a[o] = fmaf(v0[c + 3], w.w, a[o]);
      }
      __builtin_amdgcn_sched_barrier(0);  // keep the weight reads of one channel group together (register pressure)
    }
#pragma unroll
    for (int o = 0; o < NOUT; ++o) s_acc[(cq * NOUT + o) * 64 + px] = a[o];
    __syncthreads();
    if (!live) continue;  // dead lanes still meet the barriers of the next task
    const int v = b * ntask + t;  // (frame, task): plane block of `hout`, key list
    const float* hbt = hb ? hb + t * NOUT : nullptr;
    auto head_value = [&](int o) {  // quarter sums in quarter order + bias: the value stored for (pixel, head channel o)
      const float s = ((s_acc[(0 * NOUT + o) * 64 + px] + s_acc[(1 * NOUT + o) * 64 + px]) + s_acc[(2 * NOUT + o) * 64 + px]) +
                      s_acc[(3 * NOUT + o) * 64 + px];
      return s + (hbt ? hbt[o] : 0.f);
    };
    for (int o = cq; o < NOUT; o += 4) hout[((size_t)v * NOUT + o) * npix + p] = head_value(o);
    // The score filter of MultiGroupHead.predict (mg_head_sessd.py:956-972; postprocess.hip: score_filter_kernel): the same float
    // operations on the same values as the stand-alone kernel reads back from `hout`, so the keys are the same set.
    if (keys && cq == 0) {
#pragma unroll
      for (int an = 0; an < 2; ++an) {
        const float sg = 1.0f / (1.0f + expf(-head_value(14 + an)));
        if (sg >= score_thresh) {
          const float r = (head_value(20 + an) + 1.0f) * 0.5f;
          const float sc = sg * (r * r * r * r);
          const unsigned aid = (unsigned)(p * 2 + an);
          const unsigned long long key = ((unsigned long long)(~__float_as_uint(sc)) << 32) | aid;
          const int slot = atomicAdd(&key_count[v], 1);
          if (slot < key_cap) keys[(size_t)v * key_cap + slot] = key;
        }
      }
    }
  }
}

}  // namespace

extern "C" {

// rpn_v1.py:60-71 + mg_head_sessd.py:217-230, 477-481 in one launch. x (B, 128, num_pixels): the last 3x3 layer's output; up_w
// (128, 128) = the ConvTranspose2d(128, 128, 1, stride=1) weight as stored, [cin][cout]; up_scale / up_shift (128): the folded
// BatchNorm behind it (ReLU follows). head_w (num_tasks * 22, 128) row-major, head_b (num_tasks * 22) or null, head_out
// (B, num_tasks, 22, num_pixels) planar; out (B, 128, num_pixels) receives the neck's output when not null. keys / key_cap /
// key_count: as sessd_ssfa_fuse_head_tasks (per (frame, task), counts zeroed by the caller; keys == NULL: no score filter).
// channels == 128 and 1 <= num_tasks <= 4, otherwise SESSD_EINVAL.
int sessd_rpn_up_head_tasks(const float* x, const float* up_w, const float* up_scale, const float* up_shift, int batch, int channels,
                            int num_pixels, float* out, const float* head_w, const float* head_b, int num_tasks, float* head_out,
                            float score_thresh, unsigned long long* keys, int key_cap, int* key_count, hipStream_t stream) {
  if (batch < 1 || batch > 65535 || channels != 128 || num_pixels < 1 || num_tasks < 1 || num_tasks > 4) return SESSD_EINVAL;
  if (!x || !up_w || !up_scale || !up_shift || !head_w || !head_out) return SESSD_EINVAL;
  if ((long long)channels * num_pixels * 4 >= 0x7fffffffLL) return SESSD_EINVAL;  // 32-bit buffer offsets per batch element
  if ((keys == nullptr) != (key_count == nullptr) || (keys && key_cap < 1)) return SESSD_EINVAL;
  const dim3 grid(sessd_divup(num_pixels, 64), batch);
  SESSD_LAUNCH((rpn_up_head_kernel<22>), grid, dim3(256), 0, stream, x, up_w, up_scale, up_shift, num_pixels, out, head_w, head_b,
               head_out, score_thresh, keys, key_cap, key_count, num_tasks);
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}

}  // extern "C"
