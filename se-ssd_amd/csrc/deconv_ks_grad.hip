// Data and weight gradient of the kernel-size = stride transposed convolution of csrc/deconv_ks.hip (the RPN's up-samplers,
// det3d/models/necks/rpn_v1.py:84-105), s in {1, 2, 4}, cin even, cout % 32 == 0, any H, W >= 1, contiguous NCHW float32:
//     forward  out[b][o][s*y + py][s*x + px] = sum_i in[b][i][y][x] * W[i][o][py][px]
//     dgrad    gin[b][i][y][x]               = sum_{o, py, px} gout[b][o][s*y + py][s*x + px] * W[i][o][py][px]
//     wgrad    gW[i][o][py][px]              = sum_{b, y, x} in[b][i][y][x] * gout[b][o][s*y + py][s*x + px]
// Both are GEMMs on the exact-f32 matrix cores (v_mfma_f32_32x32x2_f32) in the direct-to-register form of deconv_ks.hip: operands
// go L2 / L1 -> VGPR through buffer loads, an element that does not exist is an out-of-range offset (the hardware returns 0), no LDS,
// no barrier, no atomics.
//
// dgrad: M = B*H*W pixels, N = cin, K = cout * s * s. A wave owns 32 CONSECUTIVE pixels of one image (a tile may straddle rows:
// every lane addresses its own pixel) and NT <= 4 accumulator tiles of 32 cins; the four waves of a workgroup are four pixel
// tiles over the same cins (they read the same weight lines). The B operand is gout: lane (j, h) = (lane & 31, lane >> 5) loads the
// s consecutive floats of pixel j in output row s*y + py of cout 2*op + h as float / float2 / float4 -- all px taps in one load,
// the MFMA's two k halves are two couts. The A operand is the weight, lane (i, h) = cin i of cout 2*op + h, again one s-vector.
// A k-step (one py, one cout pair) is one gout load, NT weight loads and s * NT MFMAs; the steps run py-major, two register sets
// deep. Weight copy (ops.pack_deconv_ks_dgrad), floats:  [py][cout / 2][cout parity][cin][px]
// -- a half wave reads 32 * s adjacent floats, a k-step advances by 2 * cin * s floats. Cins beyond cin load zeros and are not
// stored; pixels beyond H*W load zeros and are not stored.
//
// wgrad: the reduction axis is the pixels, the tile grid (cin x cout x s*s) is tiny, so the parallelism comes from chunks of
// pixels: a STAGE is 8 consecutive pixels of one image plane (the last stage of an image is part full), a wave accumulates one
// chunk of stages -- chunk c of n owns stages [c * stages / n, (c + 1) * stages / n) of the B * ceil(H*W / 8) stages -- into its own
// partial in the workspace, and a second kernel adds the partials IN CHUNK ORDER: the same bits on every call.
//     n = min(stages, clamp(2048 / tiles, 8, 128)),  workspace = n * cin * cout * s * s floats (partials in the stored layout)
// A wave owns one py and four 32 x 32 accumulator tiles (64 registers):
//     s = 4: the 4 px of one (cin, cout) block     s = 2: 2 px x two cin blocks     s = 1: two cin x two cout blocks
// Rows of the MFMA are cins, columns couts, the k index a pixel pair: lane (i, h) loads pixels p0 + 4h .. p0 + 4h + 3 of cin i in
// one 16-byte load (dword aligned: H*W may be odd) and, for the same four pixels of cout i, the s floats of output row s*y + py
// each (s = 1: one 16-byte load); step c of the stage multiplies the pair {p0 + c, p0 + 4 + c}. Pixels past the plane are zeroed
// in BOTH operands (the in load would otherwise run on into the next channel). The result is written in the STORED layout
// (cin, cout, s, s).
#include "common.hpp"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;
typedef __amdgpu_buffer_rsrc_t rsrc_t;

__device__ __forceinline__ rsrc_t dg_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}
constexpr unsigned DG_OOB = 0x80000000u;  // beyond any buffer: the load returns 0

// the s consecutive floats at byte offset voff + soff, into v[0 .. S)
template <int S>
__device__ __forceinline__ void dg_load(rsrc_t r, unsigned voff, unsigned soff, float* v) {
  if constexpr (S == 1) {
    v[0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0));
  } else if constexpr (S == 2) {
    const f32x2 t = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, (int)soff, 0));
    v[0] = t.x; v[1] = t.y;
  } else {
    const f32x4 t = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
}

// Four consecutive floats of a plane of which `left` exist (left >= 4: one 16-byte load; fewer: one load per float that exists, the
// others 0 -- a 16-byte load would run on into the next channel, or past the end of the tensor). voff == DG_OOB: zeros.
__device__ __forceinline__ void dw_load4(rsrc_t r, unsigned voff, int left, float* v) {
  if (left >= 4 || voff == DG_OOB) {
    dg_load<4>(r, voff, 0u, v);
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) dg_load<1>(r, c < left ? voff + 4u * c : DG_OOB, 0u, v + c);
  }
}

// ------------------------------------------------------------------ data gradient
struct DgArgs {
  const float* gout;  // (B, cout, s*h, s*w)
  const float* wpk;   // [s][cout/2][2][cin][s]
  float* gin;         // (B, cin, h, w)
  int cin, h, w, cout;
};

template <int S, int NT>
__global__ __launch_bounds__(256) void deconv_ks_dgrad_kernel(DgArgs A) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 31, hh = lane >> 5;
  const int ptile = blockIdx.x * 4 + wave, cb0 = blockIdx.y * NT, b = blockIdx.z;
  const int plane = A.h * A.w;
  if (ptile * 32 >= plane) return;  // no barrier anywhere: a wave without work leaves
  const int p = ptile * 32 + j;
  const bool live = p < plane;
  const int y = p / A.w, x = p - y * A.w;
  const int wout = S * A.w;
  const unsigned oplane = (unsigned)(S * A.h) * (unsigned)wout;
  const int KP = A.cout >> 1;

  const rsrc_t gr = dg_rsrc(A.gout + (size_t)b * A.cout * oplane, (unsigned)A.cout * oplane * 4u);
  const rsrc_t wr = dg_rsrc(A.wpk, (unsigned)A.cin * A.cout * (S * S) * 4u);
  const unsigned go = live ? ((unsigned)hh * oplane + (unsigned)(S * y) * wout + (unsigned)(S * x)) * 4u : DG_OOB;
  unsigned wo[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int c = (cb0 + n) * 32 + j;  // a cin beyond cin: zeros, never stored
    wo[n] = c < A.cin ? (unsigned)((hh * A.cin + c) * S) * 4u : DG_OOB;
  }
  const unsigned gstep = 2u * oplane * 4u, grow = (unsigned)wout * 4u, wstep = 2u * (unsigned)A.cin * S * 4u;

  f32x16 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
  float wa[2][NT][S], gb[2][S];

#define DG_LOAD(SET, KPI)                                                                          \
  {                                                                                                \
    const unsigned gs = gs0 + (unsigned)(KPI)*gstep, ws = ws0 + (unsigned)(KPI)*wstep;             \
    dg_load<S>(gr, go, gs, gb[SET]);                                                               \
    _Pragma("unroll") for (int n = 0; n < NT; ++n) dg_load<S>(wr, wo[n], ws, wa[SET][n]);          \
  }
#define DG_MMA(SET)                                                                                \
  {                                                                                                \
    _Pragma("unroll") for (int px = 0; px < S; ++px)                                               \
      _Pragma("unroll") for (int n = 0; n < NT; ++n)                                               \
        acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[SET][n][px], gb[SET][px], acc[n], 0, 0, 0); \
  }
  // per py: cout / 2 k-steps (an even number: cout % 32 == 0), two register sets, one cout pair of look-ahead; every load
  // unconditional (the last one clamped and unused), as in deconv_ks_kernel
  for (int py = 0; py < S; ++py) {
    const unsigned gs0 = (unsigned)py * grow, ws0 = (unsigned)(py * KP) * wstep;
    DG_LOAD(0, 0)
    for (int kp = 0; kp + 2 <= KP; kp += 2) {
      DG_LOAD(1, kp + 1)
      __builtin_amdgcn_sched_barrier(0);
      DG_MMA(0)
      __builtin_amdgcn_sched_barrier(0);
      DG_LOAD(0, min(kp + 2, KP - 1))
      __builtin_amdgcn_sched_barrier(0);
      DG_MMA(1)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#undef DG_LOAD
#undef DG_MMA

  // D layout (32 x 32): column = lane & 31 (pixel), row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) (cin of the block)
  if (!live) return;
  float* dst = A.gin + (size_t)b * A.cin * plane + p;
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = (cb0 + n) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
      if (c < A.cin) dst[(size_t)c * plane] = acc[n][r];
    }
}

template <int S>
int dgrad_launch(const DgArgs& A, int batch, hipStream_t stream) {
  const int ntile = sessd_divup(A.h * A.w, 32), ncb = sessd_divup(A.cin, 32);
  const dim3 block(256);
  if (ncb == 1) {
    SESSD_LAUNCH((deconv_ks_dgrad_kernel<S, 1>), dim3(sessd_divup(ntile, 4), 1, batch), block, 0, stream, A);
  } else if (ncb == 2) {
    SESSD_LAUNCH((deconv_ks_dgrad_kernel<S, 2>), dim3(sessd_divup(ntile, 4), 1, batch), block, 0, stream, A);
  } else {
    SESSD_LAUNCH((deconv_ks_dgrad_kernel<S, 4>), dim3(sessd_divup(ntile, 4), sessd_divup(ncb, 4), batch), block, 0, stream, A);
  }
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}

// ------------------------------------------------------------------ weight gradient
struct DwArgs {
  const float* in;    // (B, cin, h, w)
  const float* gout;  // (B, cout, s*h, s*w)
  float* partial;     // [nchunks][cin][cout][s][s]
  int batch, cin, h, w, cout;
  int nchunks, spi, stages;  // stages per image, stages in all
  int cot_n;                 // cout tiles of the grid
};

template <int S>
struct DwTile {
  static constexpr int CI = S == 4 ? 1 : 2;  // 32-cin blocks of a wave
  static constexpr int CO = S == 1 ? 2 : 1;  // 32-cout blocks of a wave
};

template <int S>
__global__ __launch_bounds__(64) void deconv_ks_wgrad_partial_kernel(DwArgs A) {
  constexpr int CI = DwTile<S>::CI, CO = DwTile<S>::CO;
  const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
  const int py = blockIdx.x % S, t2 = blockIdx.x / S;
  const int cot = t2 % A.cot_n, cit = t2 / A.cot_n;
  const int chunk = blockIdx.y;
  const int st0 = (int)((long long)chunk * A.stages / A.nchunks), st1 = (int)((long long)(chunk + 1) * A.stages / A.nchunks);
  const int plane = A.h * A.w, hs = S * A.h, ws = S * A.w;
  const rsrc_t xr = dg_rsrc(A.in, (unsigned)((size_t)A.batch * A.cin * plane * 4));
  const rsrc_t gr = dg_rsrc(A.gout, (unsigned)((size_t)A.batch * A.cout * hs * ws * 4));
  int ci[CI], co[CO];
#pragma unroll
  for (int m = 0; m < CI; ++m) ci[m] = (cit * CI + m) * 32 + i;
#pragma unroll
  for (int n = 0; n < CO; ++n) co[n] = (cot * CO + n) * 32 + i;

  f32x16 acc[CI][CO][S];
#pragma unroll
  for (int m = 0; m < CI; ++m)
#pragma unroll
    for (int n = 0; n < CO; ++n)
#pragma unroll
      for (int px = 0; px < S; ++px)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[m][n][px][e] = 0.f;

  // The loader walks (image, stage of the image) incrementally; a stage past the chunk loads zeros. Two register sets: the
  // operands of the next stage are fetched before the 16 MFMAs of the current one.
  float a[2][CI][4], bt[2][CO][4][S];
  int l_b = st0 / A.spi, l_q = st0 - l_b * A.spi, l_left = st1 - st0;
#define DW_LOAD(SET)                                                                                              \
  {                                                                                                               \
    const int pb = l_q * 8 + 4 * h;                                                                               \
    const bool ok = l_left > 0 && pb < plane;                                                                     \
    _Pragma("unroll") for (int m = 0; m < CI; ++m) {                                                              \
      dw_load4(xr, (ok && ci[m] < A.cin) ? (unsigned)((l_b * A.cin + ci[m]) * plane + pb) * 4u : DG_OOB, plane - pb, a[SET][m]); \
    }                                                                                                             \
    if constexpr (S == 1) {                                                                                       \
      _Pragma("unroll") for (int n = 0; n < CO; ++n) {                                                            \
        float t[4];                                                                                               \
        dw_load4(gr, (ok && co[n] < A.cout) ? (unsigned)((l_b * A.cout + co[n]) * plane + pb) * 4u : DG_OOB, plane - pb, t); \
        _Pragma("unroll") for (int c = 0; c < 4; ++c) bt[SET][n][c][0] = t[c];                                    \
      }                                                                                                           \
    } else {                                                                                                      \
      int y = pb / A.w, x = pb - y * A.w;                                                                         \
      _Pragma("unroll") for (int c = 0; c < 4; ++c) {                                                             \
        const bool in = ok && pb + c < plane;                                                                     \
        _Pragma("unroll") for (int n = 0; n < CO; ++n)                                                            \
          dg_load<S>(gr, (in && co[n] < A.cout) ? (unsigned)(((l_b * A.cout + co[n]) * hs + S * y + py) * ws + S * x) * 4u : DG_OOB, \
                     0u, bt[SET][n][c]);                                                                          \
        if (++x == A.w) { x = 0; ++y; }                                                                           \
      }                                                                                                           \
    }                                                                                                             \
    --l_left;                                                                                                     \
    if (++l_q == A.spi) { l_q = 0; ++l_b; }                                                                       \
  }
#define DW_MMA(SET)                                                                                               \
  _Pragma("unroll") for (int c = 0; c < 4; ++c)                                                                   \
    _Pragma("unroll") for (int m = 0; m < CI; ++m)                                                                \
      _Pragma("unroll") for (int n = 0; n < CO; ++n)                                                              \
        _Pragma("unroll") for (int px = 0; px < S; ++px)                                                          \
          acc[m][n][px] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[SET][m][c], bt[SET][n][c][px], acc[m][n][px], 0, 0, 0);
  DW_LOAD(0)
  for (int s = st0; s < st1; s += 2) {
    DW_LOAD(1)
    __builtin_amdgcn_sched_barrier(0);
    DW_MMA(0)
    __builtin_amdgcn_sched_barrier(0);
    DW_LOAD(0)
    __builtin_amdgcn_sched_barrier(0);
    DW_MMA(1)
    __builtin_amdgcn_sched_barrier(0);
  }
#undef DW_LOAD
#undef DW_MMA

  // D layout: column (cout) = lane & 31, row (cin) = (e & 3) + 8 * (e >> 2) + 4 * h; a lane holds all px of its (cin, cout, py)
  float* dst = A.partial + (size_t)chunk * A.cin * A.cout * (S * S);
#pragma unroll
  for (int m = 0; m < CI; ++m)
#pragma unroll
    for (int n = 0; n < CO; ++n) {
      if (co[n] >= A.cout) continue;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int cir = (cit * CI + m) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (cir >= A.cin) continue;
        float* q = dst + (((size_t)cir * A.cout + co[n]) * S + py) * S;
        if constexpr (S == 1) *q = acc[m][n][0][e];
        if constexpr (S == 2) *reinterpret_cast<float2*>(q) = make_float2(acc[m][n][0][e], acc[m][n][1][e]);
        if constexpr (S == 4)
          *reinterpret_cast<float4*>(q) = make_float4(acc[m][n][0][e], acc[m][n][1][e], acc[m][n][2][e], acc[m][n][3][e]);
      }
    }
}

__global__ __launch_bounds__(256) void deconv_ks_wgrad_reduce_kernel(const float* __restrict__ partial, int nchunks, int total,
                                                                      float* __restrict__ gw) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  // 16 loads in flight, added in chunk order (conv_wgrad_reduce_kernel of dense_grad.hip)
  float s = 0.f;
  for (int c0 = 0; c0 < nchunks; c0 += 16) {
    float v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = c0 + k < nchunks ? partial[(size_t)(c0 + k) * total + e] : 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += v[k];
  }
  gw[e] = s;
}

constexpr int DW_MAX_CHUNKS = 128;

bool dk_domain(int batch, int cin, int hin, int win, int cout, int s) {
  if (s != 1 && s != 2 && s != 4) return false;
  return !(batch < 0 || hin < 0 || win < 0 || cin < 2 || (cin & 1) || cout < 32 || (cout & 31) || batch > 65535);
}

// the chunk rule of the header comment; 1 for an empty call (so that the workspace size is never 0 inside the domain)
int dw_chunks(int batch, int cin, int hin, int win, int cout, int s, int* spi, long long* stages) {
  const int cit_n = sessd_divup(cin, 32 * (s == 4 ? 1 : 2)), cot_n = sessd_divup(cout, 32 * (s == 1 ? 2 : 1));
  const long long tiles = (long long)cit_n * cot_n * s;
  *spi = (int)(((long long)hin * win + 7) / 8);
  *stages = (long long)batch * *spi;
  long long n = 2048 / tiles;
  n = n < 8 ? 8 : (n > DW_MAX_CHUNKS ? DW_MAX_CHUNKS : n);
  if (n > *stages) n = *stages;
  return n < 1 ? 1 : (int)n;
}

}  // namespace

extern "C" {

int sessd_deconv_ks_dgrad(const float* grad_out, int batch, int cin, int hin, int win, const float* wpk, int s, int cout,
                          float* grad_in, hipStream_t stream) {
  if (!dk_domain(batch, cin, hin, win, cout, s)) return SESSD_EINVAL;
  const long long plane = (long long)hin * win;
  if (plane * batch == 0) return SESSD_OK;
  if (grad_out == nullptr || wpk == nullptr || grad_in == nullptr) return SESSD_EINVAL;
  // the buffer resources address one image's grad_out and the whole weight copy with 32-bit byte offsets; pixel indices are ints
  if (plane * s * s * cout * 4 >= (1ll << 31) || (long long)cin * cout * s * s * 4 >= (1ll << 31) || plane >= (1ll << 31) - 32)
    return SESSD_EINVAL;
  if ((((uintptr_t)grad_out | (uintptr_t)wpk) & (uintptr_t)(4 * s - 1)) != 0) return SESSD_EINVAL;  // the float2 / float4 loads
  DgArgs A;
  A.gout = grad_out; A.wpk = wpk; A.gin = grad_in;
  A.cin = cin; A.h = hin; A.w = win; A.cout = cout;
  return s == 1 ? dgrad_launch<1>(A, batch, stream) : s == 2 ? dgrad_launch<2>(A, batch, stream) : dgrad_launch<4>(A, batch, stream);
}

size_t sessd_deconv_ks_wgrad_workspace_bytes(int batch, int cin, int hin, int win, int cout, int s) {
  if (!dk_domain(batch, cin, hin, win, cout, s)) return 0;
  int spi;
  long long stages;
  const int n = dw_chunks(batch, cin, hin, win, cout, s, &spi, &stages);
  return (size_t)n * cin * cout * s * s * sizeof(float);
}

int sessd_deconv_ks_wgrad(const float* in, const float* grad_out, int batch, int cin, int hin, int win, int cout, int s,
                          float* grad_weight, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!dk_domain(batch, cin, hin, win, cout, s)) return SESSD_EINVAL;
  const long long plane = (long long)hin * win;
  if (plane * batch == 0) return SESSD_OK;
  if (in == nullptr || grad_out == nullptr || grad_weight == nullptr || workspace == nullptr) return SESSD_EINVAL;
  // the buffer resources address the WHOLE input and grad_out with 32-bit byte offsets; the reduce kernel indexes gW with an int
  if (plane * batch * cin * 4 >= (1ll << 31) || plane * batch * s * s * cout * 4 >= (1ll << 31) ||
      (long long)cin * cout * s * s * 4 >= (1ll << 31))
    return SESSD_EINVAL;
  if (((uintptr_t)grad_out & (uintptr_t)(4 * s - 1)) != 0 || ((uintptr_t)workspace & 15) != 0) return SESSD_EINVAL;
  if (workspace_bytes < sessd_deconv_ks_wgrad_workspace_bytes(batch, cin, hin, win, cout, s)) return SESSD_EINVAL;
  DwArgs A;
  A.in = in; A.gout = grad_out; A.partial = (float*)workspace;
  A.batch = batch; A.cin = cin; A.h = hin; A.w = win; A.cout = cout;
  long long stages;
  A.nchunks = dw_chunks(batch, cin, hin, win, cout, s, &A.spi, &stages);
  A.stages = (int)stages;
  const int cit_n = sessd_divup(cin, 32 * (s == 4 ? 1 : 2));
  A.cot_n = sessd_divup(cout, 32 * (s == 1 ? 2 : 1));
  const dim3 grid(cit_n * A.cot_n * s, A.nchunks), block(64);
  if (s == 1) {
    SESSD_LAUNCH(deconv_ks_wgrad_partial_kernel<1>, grid, block, 0, stream, A);
  } else if (s == 2) {
    SESSD_LAUNCH(deconv_ks_wgrad_partial_kernel<2>, grid, block, 0, stream, A);
  } else {
    SESSD_LAUNCH(deconv_ks_wgrad_partial_kernel<4>, grid, block, 0, stream, A);
  }
  SESSD_CHECK_LAUNCH();
  const int total = cin * cout * s * s;
  SESSD_LAUNCH(deconv_ks_wgrad_reduce_kernel, dim3(sessd_divup(total, 256)), dim3(256), 0, stream, (const float*)workspace,
               A.nchunks, total, grad_weight);
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}

}  // extern "C"
