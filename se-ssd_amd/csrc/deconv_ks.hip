// Kernel-size = stride transposed convolution into a channel slice of a wider NCHW map, ONE launch:
//     out[b][c_off + o][s*y + py][s*x + px] = act(scale[o] * sum_i in[b][i][y][x] * W[i][o][py][px] + shift[o]),  s in {1, 2, 4}
// Replaces nn.ConvTranspose2d(cin, cout, s, stride=s, bias=False) + BatchNorm2d + ReLU of the RPN's up-samplers
// (det3d/models/necks/rpn_v1.py:84-105) AND the torch.cat of their outputs (:116): every up-sampler writes its own channels
// [c_off, c_off + cout) of the (B, c_total, s*H, s*W) neck map; no other element of `out` is touched.
//
// A GEMM with M = B*H*W pixels, N = cout * s * s, K = cin on the exact-f32 matrix cores (v_mfma_f32_32x32x2_f32), in the
// direct-to-register form of dense_conv.hip: the A operand is the packed weight (lane (i, h) = (lane & 31, lane >> 5) holds cout
// i of cin parity h), the B operand 32 CONSECUTIVE pixels of one channel plane (one 128-byte line per half wave); operands go
// L2 / L1 -> VGPR through buffer loads whose per-k-step advance is a scalar offset, no LDS, no barrier.
//
// A wave owns one output-row parity py, 32 pixels and FOUR 32 x 32 accumulator tiles (64 registers):
//     s = 4: the 4 px of one 32-cout block        s = 2: the 2 px of two cout blocks        s = 1: four cout blocks
// so that a k-step is one activation load, four weight loads and four MFMAs for every s, and a lane (= one input pixel) holds the
// accumulators of ALL px of its pixel: per (cout, output row) it stores s consecutive floats as float / float2 / float4 -- for
// s = 4 a half wave's store is 512 contiguous bytes. The four waves of a workgroup:
//     s = 4: py = 0..3 of one pixel tile and one cout block (the four waves read the same activation lines, L1 hits)
//     s = 2: py = 0..1 x two cout groups of 64 (128 couts per workgroup)
//     s = 1: four pixel tiles x 128 couts
// Packed weight (ops.pack_deconv_ks_slice), floats:  [py][cout / 32][cin / 2][px][cin parity][32 couts]
// -- the 4 * s * 64 floats a wave reads per k-step are s adjacent 256-byte rows per cout block.
// Guards: the pixels beyond H*W of the last tile load through an out-of-range buffer offset (0) and are not stored; a tile may
// straddle image rows (every lane addresses its own pixel). Numerics: bit for bit an fmaf chain over cin in order.
#include "common.hpp"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
typedef __amdgpu_buffer_rsrc_t rsrc_t;

__device__ __forceinline__ rsrc_t dk_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float dk_load(rsrc_t rsrc, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)voff, (int)soff, 0));
}
constexpr unsigned DK_OOB = 0x80000000u;  // beyond any buffer: the load returns 0

struct DkArgs {
  const float* in;     // (B, cin, h, w)
  const float* wpk;    // [s][cout/32][cin/2][s][2][32]
  float* out;          // (B, c_total, s*h, s*w)
  const float* scale;  // [cout] or null
  const float* shift;  // [cout] or null
  int cin, h, w, cout, c_total, c_off, relu;
};

template <int S>
struct DkVec;
template <>
struct DkVec<1> { using type = float; };
template <>
struct DkVec<2> { using type = float2; };
template <>
struct DkVec<4> { using type = float4; };

template <int S>
__global__ __launch_bounds__(256) void deconv_ks_kernel(DkArgs A) {
  constexpr int CT = 4 / S;  // cout blocks of a wave
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 31, hh = lane >> 5;
  const int py = wave % S, e = wave / S;
  const int ncb = A.cout >> 5;
  int ptile = blockIdx.x, cgrp = blockIdx.y;
  if (S == 1) ptile = ptile * 4 + e;
  if (S == 2) cgrp = cgrp * 2 + e;
  const int cb0 = cgrp * CT;
  const int plane = A.h * A.w;
  const int p = ptile * 32 + j;
  if (ptile * 32 >= plane || cb0 >= ncb) return;  // no barrier anywhere: a wave without work leaves
  const int b = blockIdx.z;
  const bool live = p < plane;
  const int KP = A.cin >> 1;

  const rsrc_t xr = dk_rsrc(A.in + (size_t)b * A.cin * plane, (unsigned)A.cin * plane * 4u);
  const rsrc_t wr = dk_rsrc(A.wpk, (unsigned)A.cin * A.cout * (S * S) * 4u);
  const unsigned xo = live ? (unsigned)(hh * plane + p) * 4u : DK_OOB;
  unsigned wo[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int cb = min(cb0 + n / S, ncb - 1), px = n % S;  // a block beyond cout: loaded clamped, never stored
    wo[n] = (unsigned)((((py * ncb + cb) * KP) * S + px) * 64 + hh * 32 + j) * 4u;
  }
  const unsigned xstep = 2u * (unsigned)plane * 4u, wstep = (unsigned)S * 64u * 4u;

  f32x16 acc[4];
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
  float wa[2][4], xb[2];

#define DK_LOAD(SET, KPI)                                                                  \
  {                                                                                        \
    const unsigned ws = (unsigned)(KPI)*wstep, xs = (unsigned)(KPI)*xstep;                  \
    xb[SET] = dk_load(xr, xo, xs);                                                         \
    _Pragma("unroll") for (int n = 0; n < 4; ++n) wa[SET][n] = dk_load(wr, wo[n], ws);     \
  }
#define DK_MMA(SET)                                                                        \
  {                                                                                        \
    _Pragma("unroll") for (int n = 0; n < 4; ++n)                                          \
      acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[SET][n], xb[SET], acc[n], 0, 0, 0); \
  }
  // two register sets, one cin pair of look-ahead; every load unconditional (the last one clamped and unused), as in conv_body
  DK_LOAD(0, 0)
  for (int kp = 0; kp + 2 <= KP; kp += 2) {
    DK_LOAD(1, kp + 1)
    __builtin_amdgcn_sched_barrier(0);
    DK_MMA(0)
    __builtin_amdgcn_sched_barrier(0);
    DK_LOAD(0, min(kp + 2, KP - 1))
    __builtin_amdgcn_sched_barrier(0);
    DK_MMA(1)
    __builtin_amdgcn_sched_barrier(0);
  }
  if (KP & 1) DK_MMA(0)
#undef DK_LOAD
#undef DK_MMA

  // epilogue. D layout (32 x 32): column = lane & 31 (pixel), row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) (cout of the block).
  if (!live) return;
  using vec_t = typename DkVec<S>::type;
  const int y = p / A.w, x = p - y * A.w;
  const int wout = S * A.w;
  const size_t oplane = (size_t)(S * A.h) * wout;
  float* orow = A.out + ((size_t)b * A.c_total + A.c_off) * oplane + (size_t)(S * y + py) * wout + S * x;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    if (cb0 + c >= ncb) break;
    const int o0 = (cb0 + c) * 32 + 4 * hh;
    float sc[16], sh[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = o0 + (r & 3) + 8 * (r >> 2);
      sc[r] = A.scale ? A.scale[o] : 1.f;
      sh[r] = A.shift ? A.shift[o] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = o0 + (r & 3) + 8 * (r >> 2);
      float v[S];
#pragma unroll
      for (int px = 0; px < S; ++px) {
        v[px] = fmaf(acc[c * S + px][r], sc[r], sh[r]);
        if (A.relu) v[px] = fmaxf(v[px], 0.f);
      }
      vec_t* dst = reinterpret_cast<vec_t*>(orow + (size_t)o * oplane);
      if constexpr (S == 1) *dst = v[0];
      if constexpr (S == 2) *dst = make_float2(v[0], v[1]);
      if constexpr (S == 4) *dst = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

}  // namespace

extern "C" int sessd_deconv_ks_slice(const float* in, int batch, int cin, int hin, int win, const float* wpk, int s, float* out,
                                     int cout, int c_total, int c_off, const float* scale, const float* shift, int relu,
                                     hipStream_t stream) {
  if (s != 1 && s != 2 && s != 4) return SESSD_EINVAL;
  if (batch < 0 || hin < 0 || win < 0 || cin < 2 || (cin & 1) || cout < 32 || (cout & 31)) return SESSD_EINVAL;
  if (c_off < 0 || c_total < 1 || (long long)c_off + cout > c_total) return SESSD_EINVAL;
  const long long plane = (long long)hin * win;
  if (plane * batch == 0) return SESSD_OK;
  if (in == nullptr || wpk == nullptr || out == nullptr) return SESSD_EINVAL;
  // the buffer resources address one image's input and the whole packed weight with 32-bit byte offsets
  if (plane * cin * 4 >= (1ll << 31) || (long long)cin * cout * s * s * 4 >= (1ll << 31)) return SESSD_EINVAL;
  if (batch > 65535) return SESSD_EINVAL;
  if (((uintptr_t)out & (uintptr_t)(4 * s - 1)) != 0) return SESSD_EINVAL;  // the float2 / float4 stores
  DkArgs A;
  A.in = in; A.wpk = wpk; A.out = out; A.scale = scale; A.shift = shift;
  A.cin = cin; A.h = hin; A.w = win; A.cout = cout; A.c_total = c_total; A.c_off = c_off; A.relu = relu ? 1 : 0;
  const int ntile = (int)((plane + 31) / 32), ncb = cout / 32;
  if (s == 1) {
    SESSD_LAUNCH(deconv_ks_kernel<1>, dim3(sessd_divup(ntile, 4), sessd_divup(ncb, 4), batch), dim3(256), 0, stream, A);
  } else if (s == 2) {
    SESSD_LAUNCH(deconv_ks_kernel<2>, dim3(ntile, sessd_divup(ncb, 4), batch), dim3(256), 0, stream, A);
  } else {
    SESSD_LAUNCH(deconv_ks_kernel<4>, dim3(ntile, ncb, batch), dim3(256), 0, stream, A);
  }
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}
