// bottom_up_block_1's first layer of the SSFA neck over a tile list on the bf16 matrix cores at f32 accuracy: Conv2d(cin, cout, 3,
// stride 2, padding 1) + folded BatchNorm + ReLU (+ residual, added after the ReLU) (det3d/models/necks/rpn_v1.py). Contract of
// sessd_conv2d_sk_active for this layer: for each listed 2x2 tile of the OUTPUT map its four pixels, all couts; the other output
// pixels are not touched.
//
//     out(oy, ox) = sum over (ky, kx) of W[:, :, ky, kx] in(2 oy - 1 + ky, 2 ox - 1 + kx)        (0 outside the image)
//
// a (128 couts) x (pixels) x (9 cin) GEMM. The f32 kernel (conv2d_sk_kernel<true>, tile_cfg 30) is matrix-pipe bound on 64-cycle
// f32 MFMAs and has 56 units of 128 x 128 for the layer's list, so stream-K cuts nearly all of them and their partial tiles
// travel through memory. Here, as in dense_deconv_split.hip, every operand is split into three bf16 terms a = a0 + a1 + a2
// (bf16_split.hpp) and the six products with i + j <= 2 are kept, smallest first: a2b0, a1b1, a0b2, a1b0, a0b1, a0b0 -- one K = 16
// v_mfma_f32_32x32x16_bf16 each.
//
//   unit      = 16 list entries (64 output pixels) x 128 couts x all cin and taps. Whole units only: nothing is cut, no partial
//               sums through memory, no workspace, no counters. The grid is sized from list_cap; workgroups past the device count
//               leave at once, before any barrier. Neighbouring workgroups take the cout groups of the same pixels.
//   workgroup = 4 waves, one per cout block of 32; a wave holds 2 pixel blocks of 32x32 in three accumulator sets (acc, accl, tot:
//               96 registers, see "Where the sums go" below). Two workgroups fit a CU (36 KB of LDS each). Lane j of a pixel block
//               = pixel (entry j / 4, row (j / 2) % 2, column j % 2).
//   step      = one kernel row ky of one k-step of 16 input channels: 3 taps x 6 products x 2 pixel blocks = 36 MFMAs per wave.
//   weights   : packed once per model (ops.pack_conv2d_s2_split) as bf16 [cout group 128][k-step cin / 16][tap 3 ky + kx][plane 3]
//               [cout block 4][lane = (cin / 8) % 2 * 32 + cout % 32][cin % 8]: the A fragment of a (tap, plane) is one b128 load
//               per lane and feeds both pixel blocks. A ring of three taps, loaded two taps ahead (across step boundaries).
//   pixels    : per step the workgroup loads the three shifted copies (kx) of its 64 pixels in f32 (thread = (pixel block, channel
//               quarter, channel half, pixel): 3 x 4 dword buffer loads, out-of-range offsets outside the image and past the count),
//               splits each value once and writes the three planes in MFMA-B fragment order [tap 3][pixel block 2][plane 3]
//               [lane 64][8 channels] -- 18 KB per buffer, two buffers. The loads of step s + 2 are issued in step s, the split
//               and LDS stores of step s + 1 are interleaved with the MFMAs of step s's first tap, the one LDS-only barrier of a
//               step stands between its second and third tap, and the first tap's B fragments of step s + 1 are read behind it:
//               a wave waits for LDS with 12 MFMAs in the pipe.
// Numerics: per (cout, pixel) a fixed order (k-step, ky, kx, product) whatever else is listed: a listed tile's bits do not depend
// on the list, its order or the launch. Against float64 the error is at or below the f32 kernel's (tests/test_conv_s2_split_gpu.py).
// Tried and measured on MI355X (cin 128 -> cout 256, 896 listed tiles of the 100 x 88 map = 112 units, alone on the whole chip,
// against 45.5 us for the f32 stream-K kernel's best min_rounds):
//   - all six products of all steps chained on one accumulator per pixel block: error 1.65e-6 against the f32 kernel's 7.6e-7
//     at cin 16 (it failed the rule e_split <= 2 e_f32 there already);
//   - a0b0 on an accumulator of its own, chained over all steps: 35 - 37 us, error 1.7 - 2.2 x the f32 kernel's at cin 128;
//   - the shipped form (a0b0 chained per step and summed on the VALU, two rotating B-fragment sets instead of three to stay
//     inside 256 registers): 36.5 - 38.8 us, error 0.8 - 1.1 x the f32 kernel's at cin 128, 0.4 - 0.7 x at cin 16 / 32; in the
//     frame on a 128-CU set 43.7 us against 68.0.
// Resources (hipcc, gfx950, from the compiler's resource remarks): 248 VGPRs (the unified file of a wave at two waves per SIMD),
// 0 AGPRs, 72 SGPRs, no scratch, 36 KB LDS.
#include "common.hpp"
#include "bf16_split.hpp"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
typedef unsigned int u32x2g __attribute__((__vector_size__(8)));
typedef unsigned int u32x4g __attribute__((__vector_size__(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
using sessd::split3_pk;

typedef __amdgpu_buffer_rsrc_t rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float bufload(rsrc_t rsrc, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)voff, (int)soff, 0));
}
#define SESSD_OOB 0x80000000u
// workgroup barrier that orders LDS traffic only (see dense_wino_sk.hip)
#define SESSD_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

struct ConvS2SplitArgs {
  const float* in;              // (B, cin, hin, win)
  const void* w;                // the packed bf16 planes
  float* out;                   // (B, cout, hout, wout)
  const float* scale;
  const float* shift;
  const float* residual;
  const int* tile_list;         // entries image * (hout/2 * wout/2) + tile
  const int* n_list;
  int list_cap, batch, cin, hin, win, cout, hout, wout, relu, ngroups;
};

// list position k -> image and top-left OUTPUT pixel of its tile; false past the count (or for an entry outside the maps)
__device__ __forceinline__ bool tile_of(const ConvS2SplitArgs& A, int n_list, int k, int& img, int& y0, int& x0) {
  const int ntiles2 = (A.hout >> 1) * (A.wout >> 1), tw2 = A.wout >> 1;
  const int ent = k < n_list ? A.tile_list[k] : -1;
  const bool live = ent >= 0 && ent < A.batch * ntiles2;
  img = live ? ent / ntiles2 : 0;
  const int t = live ? ent - img * ntiles2 : 0;
  y0 = 2 * (t / tw2);
  x0 = 2 * (t - (t / tw2) * tw2);
  return live;
}

constexpr int XBUF = 3 * 2 * 3 * 256;   // words of one pixel buffer: [tap kx][pixel block][plane][lane][4 words]

__global__ __launch_bounds__(256, 2) void conv_s2_split_kernel(ConvS2SplitArgs A) {
  __shared__ __attribute__((aligned(16))) unsigned lds[2 * XBUF];   // 36 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int n_list = __builtin_amdgcn_readfirstlane(min(A.n_list[0], A.list_cap));
  const int unit = blockIdx.x / A.ngroups, grp = blockIdx.x - unit * A.ngroups;
  if (unit * 16 >= n_list) return;   // the whole workgroup, before any barrier

  const int npix = A.hin * A.win;
  const unsigned plane4 = (unsigned)npix * 4u;
  const int KS = A.cin >> 4;
  const rsrc_t xr = make_rsrc(A.in, (unsigned)A.batch * A.cin * plane4);
  const rsrc_t wr = make_rsrc(A.w, (unsigned)A.ngroups * KS * (27u * 4096u));

  // ---- staging: wave = (pixel block spb, channel quarter sq), lane = (channel half h, pixel j): channels 8 h + 4 sq + 0 .. 3
  const int spb = wave & 1, sq = wave >> 1;
  unsigned xo[3][3];
  {
    int img, y0, x0;
    const bool live = tile_of(A, n_list, unit * 16 + spb * 8 + (j >> 2), img, y0, x0);
    const int iy0 = 2 * (y0 + ((j >> 1) & 1)) - 1, ix0 = 2 * (x0 + (j & 1)) - 1;
    const unsigned base = (unsigned)(img * A.cin + h * 8 + sq * 4) * (unsigned)npix;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int iy = iy0 + ky, ix = ix0 + kx;
        xo[ky][kx] = (live && iy >= 0 && iy < A.hin && ix >= 0 && ix < A.win) ? (base + (unsigned)(iy * A.win + ix)) * 4u : SESSD_OOB;
      }
  }
  const int wthr = (spb * 3 * 64 + lane) * 4 + sq * 2;   // this thread's words of a buffer: fragment (tap 0, spb, plane 0) ...
  float xs[3][4];
  // the pixels of kernel row KY of k-step KSTEP (clamped past the end: loaded once more, never read)
#define SESSD_CS_LOADX(KSTEP, KY)                                                                   \
  {                                                                                                 \
    const unsigned c0 = (unsigned)min((KSTEP), KS - 1) * 16u;                                       \
    _Pragma("unroll") for (int kx = 0; kx < 3; ++kx)                                                \
      _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                 \
        xs[kx][i] = bufload(xr, xo[KY][kx], (c0 + i) * plane4);                                     \
  }
  // split xs and store the three planes of every tap at word offset VOFF
#define SESSD_CS_SPLIT_STORE(VOFF)                                                                  \
  {                                                                                                 \
    _Pragma("unroll") for (int kx = 0; kx < 3; ++kx) {                                              \
      u32x2g t0, t1, t2;                                                                            \
      _Pragma("unroll") for (int q = 0; q < 2; ++q) {                                               \
        unsigned a0, a1, a2;                                                                        \
        split3_pk(xs[kx][2 * q], xs[kx][2 * q + 1], a0, a1, a2);                                    \
        t0[q] = a0; t1[q] = a1; t2[q] = a2;                                                         \
      }                                                                                             \
      unsigned* dst = lds + (VOFF) + wthr + kx * (2 * 3 * 256);                                     \
      *static_cast<u32x2g*>(__builtin_assume_aligned(dst, 8)) = t0;                                 \
      *static_cast<u32x2g*>(__builtin_assume_aligned(dst + 256, 8)) = t1;                           \
      *static_cast<u32x2g*>(__builtin_assume_aligned(dst + 512, 8)) = t2;                           \
    }                                                                                               \
  }

  // ---- compute: wave = cout block cb
  const int cb = wave;
  const int rthr = lane * 4;
  const unsigned wvo = (unsigned)(cb * 1024 + lane * 16);
  const unsigned wgrp = (unsigned)grp * (unsigned)KS * (27u * 4096u);
  const int tlast = KS * 9 - 1;
  f32x16 acc[2], accl[2], tot[2];
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < 2; ++q) acc[q] = accl[q] = tot[q] = zero16;
  bf16x8 af[3][3], bf[2][2][3];

  // tap index TG over the whole loop (k-step * 9 + 3 ky + kx); the last loads are clamped and unused
#define SESSD_CS_LOADA(SET, TG)                                                                     \
  {                                                                                                 \
    const unsigned ws = wgrp + (unsigned)min((TG), tlast) * (3u * 4096u);                           \
    _Pragma("unroll") for (int p = 0; p < 3; ++p)                                                   \
      af[SET][p] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wr, (int)wvo, (int)(ws + 4096u * p), 0)); \
  }
  // the B fragments of tap KX (both pixel blocks, three planes) from the buffer at word offset VOFF into fragment set BS
#define SESSD_CS_READB(VOFF, KX, BS)                                                                \
  {                                                                                                 \
    _Pragma("unroll") for (int q = 0; q < 2; ++q)                                                   \
      _Pragma("unroll") for (int p = 0; p < 3; ++p)                                                 \
        bf[BS][q][p] = __builtin_bit_cast(bf16x8, *static_cast<const u32x4g*>(__builtin_assume_aligned( \
            lds + (VOFF) + rthr + (((KX)*2 + q) * 3 + p) * 256, 16)));                              \
  }
  // Where the sums go. The bf16 MFMA's accumulate is less exact than an f32 addition (measured: with all six products of all
  // steps chained on one accumulator the error against float64 is more than twice the f32 kernel's and grows with the chain), so the
  // chains are kept short where the sum is large: a0b0 of ONE step's three taps is chained from zero in acc and added to tot with
  // a VALU addition at the head of the next step (between that step's first ten MFMAs, which go to accl); the five small
  // products (2^-8 of a0b0 and below) are chained in accl, where an accumulate's error is 2^-8 of what it is in acc.
#define SESSD_CS_M(ACC, KX, BS, PA, PB)                                                             \
  _Pragma("unroll") for (int q = 0; q < 2; ++q)                                                     \
    ACC[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[KX][PA], bf[BS][q][PB], ACC[q], 0, 0, 0);
#define SESSD_CS_MSMALL(KX, BS)                                                                     \
  SESSD_CS_M(accl, KX, BS, 2, 0)                                                                    \
  SESSD_CS_M(accl, KX, BS, 1, 1)                                                                    \
  SESSD_CS_M(accl, KX, BS, 0, 2)                                                                    \
  SESSD_CS_M(accl, KX, BS, 1, 0)                                                                    \
  SESSD_CS_M(accl, KX, BS, 0, 1)
#define SESSD_CS_MMA(KX, BS)                                                                        \
  {                                                                                                 \
    SESSD_CS_MSMALL(KX, BS)                                                                         \
    SESSD_CS_M(acc, KX, BS, 0, 0)                                                                   \
  }
  // the first tap of a step: the step before leaves acc for tot, a0b0 starts from zero
#define SESSD_CS_MMA_FIRST(BS)                                                                      \
  {                                                                                                 \
    _Pragma("unroll") for (int q = 0; q < 2; ++q) tot[q] += acc[q];                                 \
    SESSD_CS_MSMALL(0, BS)                                                                          \
    _Pragma("unroll") for (int q = 0; q < 2; ++q)                                                   \
      acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][0], bf[BS][q][0], zero16, 0, 0, 0);    \
  }
  // One step = kernel row KY of k-step KS_, pixels in the buffer at voff; xs holds the pixels of the NEXT step on entry and
  // fragment set S0 this step's first tap. Two fragment sets: taps 0 and 2 use S0, tap 1 uses S1, and the next step's first tap
  // is read into S1 -- the sets swap roles from step to step. The other buffer was last read before the barrier of the step
  // before: it may be written from the start of this one. Behind this step's barrier every wave has read this buffer's taps 1
  // and 2 (tap 0 was read behind the barrier before) and written the other one.
#define SESSD_CS_STEP(KS_, KY, S0, S1)                                                              \
  {                                                                                                 \
    const int tg = (KS_)*9 + (KY)*3;                                                                \
    SESSD_CS_READB(voff, 1, S1)                                                                     \
    SESSD_CS_LOADA(2, tg + 2)                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    SESSD_CS_MMA_FIRST(S0)                                                                          \
    SESSD_CS_SPLIT_STORE(voff ^ XBUF)                                                               \
    _Pragma("unroll") for (int g = 0; g < 12; ++g) {                                                \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                            \
      __builtin_amdgcn_sched_group_barrier(0x002, 9, 0);                                            \
    }                                                                                               \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    SESSD_CS_READB(voff, 2, S0)                                                                     \
    SESSD_CS_LOADX((KS_) + ((KY) + 2) / 3, ((KY) + 2) % 3)                                          \
    SESSD_CS_LOADA(0, tg + 3)                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    SESSD_CS_MMA(1, S1)                                                                             \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    SESSD_LDS_BARRIER();                                                                            \
    voff ^= XBUF;                                                                                   \
    SESSD_CS_READB(voff, 0, S1)                                                                     \
    SESSD_CS_LOADA(1, tg + 4)                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    SESSD_CS_MMA(2, S0)                                                                             \
    __builtin_amdgcn_sched_barrier(0);                                                              \
  }

  int voff = 0;
  SESSD_CS_LOADX(0, 0)
  SESSD_CS_LOADA(0, 0)
  SESSD_CS_LOADA(1, 1)
  __builtin_amdgcn_sched_barrier(0);
  SESSD_CS_SPLIT_STORE(0)
  SESSD_CS_LOADX(0, 1)
  SESSD_LDS_BARRIER();
  SESSD_CS_READB(0, 0, 0)
  __builtin_amdgcn_sched_barrier(0);
  int ks = 0;
  for (; ks + 1 < KS; ks += 2) {   // two k-steps = six steps: the fragment sets are back in their roles
    SESSD_CS_STEP(ks, 0, 0, 1)
    SESSD_CS_STEP(ks, 1, 1, 0)
    SESSD_CS_STEP(ks, 2, 0, 1)
    SESSD_CS_STEP(ks + 1, 0, 1, 0)
    SESSD_CS_STEP(ks + 1, 1, 0, 1)
    SESSD_CS_STEP(ks + 1, 2, 1, 0)
  }
  if (ks < KS) {                   // an odd number of k-steps
    SESSD_CS_STEP(ks, 0, 0, 1)
    SESSD_CS_STEP(ks, 1, 1, 0)
    SESSD_CS_STEP(ks, 2, 0, 1)
  }
#undef SESSD_CS_LOADX
#undef SESSD_CS_SPLIT_STORE
#undef SESSD_CS_LOADA
#undef SESSD_CS_READB
#undef SESSD_CS_M
#undef SESSD_CS_MMA
#undef SESSD_CS_MSMALL
#undef SESSD_CS_MMA_FIRST
#undef SESSD_CS_STEP

  // ---- epilogue: D column = lane & 31 (pixel), row = (r & 3) + 8 (r >> 2) + 4 h (cout); an element past the count or beyond cout
  // gets an out-of-range buffer offset
  const unsigned oplane = (unsigned)(A.hout * A.wout);
  const unsigned obytes = (unsigned)A.batch * A.cout * oplane * 4u;
  const float* res = A.residual;
  const rsrc_t orr = make_rsrc(A.out, obytes);
  const rsrc_t rr = make_rsrc(res ? res : A.out, res ? obytes : 0u);
  const rsrc_t scr = make_rsrc(A.scale ? A.scale : A.in, A.scale ? (unsigned)A.cout * 4u : 0u);
  const rsrc_t shr = make_rsrc(A.shift ? A.shift : A.in, A.shift ? (unsigned)A.cout * 4u : 0u);
  const int co0 = grp * 128 + cb * 32 + 4 * h;
  float scv[16], shv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int k = (r & 3) + 8 * (r >> 2);
    scv[r] = A.scale ? bufload(scr, (unsigned)(co0 + k) * 4u, 0) : 1.f;
    shv[r] = bufload(shr, (unsigned)(co0 + k) * 4u, 0);
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    int img, y0, x0;
    const bool live = tile_of(A, n_list, unit * 16 + q * 8 + (j >> 2), img, y0, x0);
    const int y = y0 + ((j >> 1) & 1), x = x0 + (j & 1);
    const unsigned vbase = ((unsigned)(img * A.cout + co0) * oplane + (unsigned)(y * A.wout + x)) * 4u;
    unsigned vo[16];
    float rv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = (r & 3) + 8 * (r >> 2);
      vo[r] = (live && co0 + k < A.cout) ? vbase + (unsigned)k * oplane * 4u : SESSD_OOB;
      rv[r] = bufload(rr, vo[r], 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v = fmaf((tot[q][r] + acc[q][r]) + accl[q][r], scv[r], shv[r]);
      if (A.relu) v = fmaxf(v, 0.f);
      if (res) v += rv[r];
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), orr, (int)vo[r], 0, 0);
    }
  }
}

// bytes of the split weight planes
size_t split_pack_bytes(int cin, int cout) { return (size_t)sessd_divup(cout, 128) * (cin / 16) * 27 * 4096; }

}  // namespace

extern "C" {

// Conv2d(cin, cout, 3, stride 2, padding 1) + epilogue over the listed 2x2 tiles of its output map, on the bf16 matrix cores with
// three-way split operands (f32 accuracy). wsplit: the weight as three bf16 planes in fragment order (ops.pack_conv2d_s2_split:
// ceil(cout / 128) * cin / 16 * 27 * 4096 bytes). cin % 16 == 0, even hout / wout, hin in {2 hout - 1, 2 hout} and win likewise,
// the whole batch inside 32-bit offsets. One workgroup of 4 waves per (16 list entries, 128 couts), two per CU; no scratch.
int sessd_conv2d_s2_split_active(const float* in, int batch, int cin, int hin, int win, const void* wsplit, float* out, int cout,
                                 int hout, int wout, const sessd_conv_epilogue_t* epilogue, const sessd_tile_list_t* list,
                                 hipStream_t stream) {
  if (cin < 16 || cin % 16 || batch < 1 || cout < 1 || hout < 2 || wout < 2 || (hout & 1) || (wout & 1)) return SESSD_EINVAL;
  if ((hin != 2 * hout && hin != 2 * hout - 1) || (win != 2 * wout && win != 2 * wout - 1)) return SESSD_EINVAL;
  if (!in || !wsplit || !out || !list || !sessd_tile_list_ok(list)) return SESSD_EINVAL;
  if ((long long)batch * cout * hout * wout * 4 >= 0x7fffffffLL || (long long)batch * cin * hin * win * 4 >= 0x7fffffffLL) return SESSD_EINVAL;
  if (split_pack_bytes(cin, cout) >= 0x7fffffffULL) return SESSD_EINVAL;
  ConvS2SplitArgs A;
  A.in = in; A.w = wsplit; A.out = out;
  sessd_take_epilogue(A, epilogue);
  sessd_take_tile_list(A, list);
  A.batch = batch; A.cin = cin; A.hin = hin; A.win = win; A.cout = cout; A.hout = hout; A.wout = wout;
  A.ngroups = sessd_divup(cout, 128);
  const long long wgs = (long long)sessd_divup(list->cap, 16) * A.ngroups;
  if (wgs > 0x7fffffffLL) return SESSD_EINVAL;
  SESSD_LAUNCH(conv_s2_split_kernel, dim3((unsigned)wgs), dim3(256), 0, stream, A);
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}

}  // extern "C"
