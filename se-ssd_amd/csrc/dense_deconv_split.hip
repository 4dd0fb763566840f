// The transposed pair of the SSFA neck over a tile list on the bf16 matrix cores at f32 accuracy: deconv_block_0 / deconv_block_1
// (det3d/models/necks/rpn_v1.py:175-199), two ConvTranspose2d(cin, cout, 3, stride 2, padding 1, output_padding 1) + folded
// BatchNorm + ReLU (+ residual, added after the ReLU) on the SAME input. Contract of sessd_deconv2d_s2_mfma_pair_active: for each
// listed 2x2 tile of the INPUT map the 4x4 output block of both layers; the other output pixels are not touched.
//
// With e = (ey, ex) and X_e = in(y + ey, x + ex) (0 outside the image) the four output parities of input pixel (y, x) are the
// nine terms of dense_deconv_pair.hip:
//     (0,0): W11 X00            (0,1): W10 X01 + W12 X00            (1,0): W01 X10 + W21 X00
//     (1,1): W00 X11 + W02 X10 + W20 X01 + W22 X00
// each a (128 couts) x (pixels) x (cin) GEMM accumulated straight into the accumulator of its parity. The f32 direct kernel
// (conv2d_mfma8_kernel) feeds every 64-cycle f32 MFMA with two global dword loads per lane and is matrix-pipe bound; here
// every operand is split into three bf16 terms a = a0 + a1 + a2 (bf16_split.hpp; each rounded to nearest from the exact residual)
// and the six products with i + j <= 2 are kept, in the order of dense_wino_sk.hip shape 3 (smallest first): a2b0, a1b1, a0b2,
// a1b0, a0b1, a0b0 -- one K = 16 v_mfma_f32_32x32x16_bf16 each.
//
//   unit      = 16 list entries (64 input pixels) x 128 couts of ONE layer x all cin. Whole units only: nothing is cut, no
//               partial sums through memory, no counters, no workgroup waits for another. The grid is sized from list_cap;
//               workgroups past the device count leave at once. Even / odd workgroups take layer a / b, so an XCD's L2 holds one
//               layer's weights.
//   workgroup = 4 waves, one per cout block of 32 (cb); a wave holds 4 parities x 2 pixel blocks of 32x32 = 8 accumulators (128
//               registers). Two workgroups per CU (48 KB of LDS and 248 registers each): one's prologue and epilogue run beside
//               the other's MFMAs. Lane j of a pixel block = pixel (entry j / 4, row (j / 2) % 2, column j % 2).
//   weights   : packed once per model (ops.pack_deconv2d_s2(w).wsplit()) as bf16 [cout group 128][k-step cin / 16][tap 9]
//               [plane 3][cb 4][lane = (cin / 8) % 2 * 32 + cout % 32][cin % 8]: the A fragment of a (tap, plane) is one b128
//               load per lane; it feeds both pixel blocks. Taps in the order they are used, grouped by e so that one set of B
//               fragments is live: W11 W12 W21 W22 (e 00), W10 W20 (e 01), W01 W02 (e 10), W00 (e 11). A ring of three taps,
//               loaded two taps ahead (across the k-step boundary).
//   pixels    : per k-step (16 input channels) the workgroup loads the four shifted copies X_e of its 64 pixels in f32 (thread
//               = (e, pixel block, channel half, pixel): 2 x 8 dword buffer loads, out-of-range offsets at the right / bottom
//               border and past the count), splits each value once and writes the three planes in MFMA-B fragment order
//               [e 4][pixel block 2][plane 3][lane 64][8 channels] -- 24 KB per buffer, two buffers. The loads of step s + 1
//               are issued before the MFMAs of step s; their split and LDS stores are interleaved with the MFMAs of taps 4 and 6
//               (four VALU instructions per MFMA gap), the B fragments of the next e group are read into the registers of the
//               current one as each plane's last use has issued; one LDS-only barrier per step. Per k-step a wave reads 24
//               ds_read_b128 for its 108 MFMAs.
//   stores    : lane = input pixel; the two px outputs of an output row leave as one 8-byte store, the residual is read the same
//               way (dense_deconv_pair.hip); every output line of a listed block is written once.
// Numerics: per (cout, pixel) a fixed order (k-step, tap, product) whatever else is listed: a listed block's bits do not depend
// on the list. Against float64 the error is that of the f32 pair kernel (tests/test_deconv_split_gpu.py).
// Measured on MI355X (1420 listed tiles of the 100 x 88 map, 256 -> 128, whole chip): 56 - 62 us per launch against 79 us for the
// f32 direct kernel's best tile_cfg; about 4.0 us per k-step. The same loop in a workgroup of 8 waves (NW = 8: 128-pixel units,
// 96 KB, one workgroup per CU) takes 88 us: a unit's prologue and epilogue (~25 us: list, first pixels, 64 scattered 8-byte
// stores per wave) then run with the CU's matrix cores idle. Resources (hipcc, gfx950): 248 VGPRs (the unified file of a wave
// at two waves per SIMD; the 128 accumulator registers among them, 0 AGPRs), 44 SGPRs, no scratch, 48 KB LDS.
#include "common.hpp"
#include "bf16_split.hpp"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x2v = __attribute__((ext_vector_type(2))) float;
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

struct DeconvSplitArgs {
  const float* in;              // (B, cin, hin, win)
  const void* w[2];             // per layer: the packed bf16 planes
  float* out[2];                // (B, cout, 2 hin, 2 win)
  const float* scale[2];
  const float* shift[2];
  const float* residual[2];
  const int* tile_list;         // entries image * (hin/2 * win/2) + tile
  const int* n_list;
  int list_cap, batch, cin, hin, win, cout, relu, ngroups;
};


// list position k -> image and top-left pixel of its tile; false past the count (or for an entry outside the maps)
__device__ __forceinline__ bool tile_of(const DeconvSplitArgs& A, int n_list, int k, int& img, int& y0, int& x0) {
  const int ntiles2 = (A.hin >> 1) * (A.win >> 1), tw2 = A.win >> 1;
  const int ent = k < n_list ? A.tile_list[k] : -1;
  const bool live = ent >= 0 && ent < A.batch * ntiles2;
  img = live ? ent / ntiles2 : 0;
  const int t = live ? ent - img * ntiles2 : 0;
  y0 = 2 * (t / tw2);
  x0 = 2 * (t - (t / tw2) * tw2);
  return live;
}

template <int NW>
__global__ __launch_bounds__(NW * 64, 8 / NW) void deconv_pair_split_kernel(DeconvSplitArgs A) {
  constexpr int NPB = NW / 2;                 // pixel blocks of a unit (two per pixel half)
  constexpr int NE = 8 * NPB;                 // list entries of a unit
  constexpr int XBUF = 4 * NPB * 3 * 256;     // words of one pixel buffer: [e][pixel block][plane][lane][4 words]
  __shared__ __attribute__((aligned(16))) unsigned lds[2 * XBUF];   // 48 KB (NW = 4)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int n_list = __builtin_amdgcn_readfirstlane(min(A.n_list[0], A.list_cap));
  const int layer = blockIdx.x & 1;
  const int rest = blockIdx.x >> 1;
  const int unit = rest / A.ngroups, grp = rest - unit * A.ngroups;
  if (unit * NE >= n_list) return;   // the whole workgroup, before any barrier

  const int npix = A.hin * A.win;
  const unsigned plane4 = (unsigned)npix * 4u;
  const int KS = A.cin >> 4;
  const rsrc_t xr = make_rsrc(A.in, (unsigned)A.batch * A.cin * plane4);
  const rsrc_t wr = make_rsrc(A.w[layer], (unsigned)A.ngroups * KS * (27u * 4096u));

  // ---- staging: items (e, pixel block) = wave and wave + 8, lane = (channel half h, pixel j)
  unsigned xo[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int idx = wave + NW * r, e = idx / NPB, pb = idx % NPB;
    int img, y0, x0;
    const bool live = tile_of(A, n_list, unit * NE + pb * 8 + (j >> 2), img, y0, x0);
    const int iy = y0 + ((j >> 1) & 1) + (e >> 1), ix = x0 + (j & 1) + (e & 1);
    xo[r] = (live && iy < A.hin && ix < A.win) ? ((unsigned)(img * A.cin + h * 8) * (unsigned)npix + (unsigned)(iy * A.win + ix)) * 4u
                                              : SESSD_OOB;
  }
  const int wthr = (wave * 3 * 64 + lane) * 4;   // this thread's words of a buffer: fragment (item, plane 0) ...
  float xs[2][8];
#define SESSD_DS_LOADX(STEP)                                                                        \
  {                                                                                                 \
    _Pragma("unroll") for (int r = 0; r < 2; ++r)                                                   \
      _Pragma("unroll") for (int i = 0; i < 8; ++i)                                                 \
        xs[r][i] = bufload(xr, xo[r], (unsigned)((STEP)*16 + i) * plane4);                          \
  }
  u32x4g tw[3];
#define SESSD_DS_SPLITX(R)                                                                          \
  {                                                                                                 \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                 \
      unsigned a0, a1, a2;                                                                          \
      split3_pk(xs[R][2 * q], xs[R][2 * q + 1], a0, a1, a2);                                        \
      tw[0][q] = a0; tw[1][q] = a1; tw[2][q] = a2;                                                  \
    }                                                                                               \
  }
#define SESSD_DS_STOREX(VOFF, R)                                                                    \
  {                                                                                                 \
    unsigned* dst = lds + (VOFF) + wthr + (R) * (NW * 3 * 256);                                      \
    *static_cast<u32x4g*>(__builtin_assume_aligned(dst, 16)) = tw[0];                               \
    *static_cast<u32x4g*>(__builtin_assume_aligned(dst + 256, 16)) = tw[1];                         \
    *static_cast<u32x4g*>(__builtin_assume_aligned(dst + 512, 16)) = tw[2];                         \
  }

  // ---- compute: wave = (cout block cb, pixel half ph); ph = 0 with four waves
  const int cb = wave & 3, ph = wave >> 2;
  const int rthr = (2 * ph * 3 * 64 + lane) * 4;   // ... and fragment (e 0, pixel block 2 ph, plane 0)
  const unsigned wvo = (unsigned)(cb * 1024 + lane * 16);
  const unsigned wgrp = (unsigned)grp * (unsigned)KS * (27u * 4096u);
  const int tlast = KS * 9 - 1;
  f32x16 acc[4][2];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][q][r] = 0.f;
  bf16x8 af[3][3], bf[2][3];

  // tap index TG over the whole k loop (k-step * 9 + tap); the last loads are clamped and unused
#define SESSD_DS_LOADA(SET, TG)                                                                     \
  {                                                                                                 \
    const unsigned ws = wgrp + (unsigned)min((TG), tlast) * (3u * 4096u);                           \
    _Pragma("unroll") for (int p = 0; p < 3; ++p)                                                   \
      af[SET][p] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wr, (int)wvo, (int)(ws + 4096u * p), 0)); \
  }
#define SESSD_DS_READB(VOFF, E)                                                                     \
  {                                                                                                 \
    _Pragma("unroll") for (int q = 0; q < 2; ++q)                                                   \
      _Pragma("unroll") for (int p = 0; p < 3; ++p)                                                 \
        bf[q][p] = __builtin_bit_cast(bf16x8, *static_cast<const u32x4g*>(__builtin_assume_aligned(  \
            lds + (VOFF) + rthr + (((E)*NPB + q) * 3 + p) * 256, 16)));                               \
  }
#define SESSD_DS_M(SET, PAR, PA, PB)                                                                \
  _Pragma("unroll") for (int q = 0; q < 2; ++q)                                                     \
    acc[PAR][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[SET][PA], bf[q][PB], acc[PAR][q], 0, 0, 0);
#define SESSD_DS_MMA(SET, PAR)                                                                      \
  {                                                                                                 \
    SESSD_DS_M(SET, PAR, 2, 0)                                                                      \
    SESSD_DS_M(SET, PAR, 1, 1)                                                                      \
    SESSD_DS_M(SET, PAR, 0, 2)                                                                      \
    SESSD_DS_M(SET, PAR, 1, 0)                                                                      \
    SESSD_DS_M(SET, PAR, 0, 1)                                                                      \
    SESSD_DS_M(SET, PAR, 0, 0)                                                                      \
  }
  // tap T of the k-step (ring set T % 3) into parity PAR; the tap two ahead is loaded first
#define SESSD_DS_TAP(T, PAR)                                                                        \
  {                                                                                                 \
    SESSD_DS_LOADA(((T) + 2) % 3, s * 9 + (T) + 2)                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    SESSD_DS_MMA((T) % 3, PAR)                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                              \
  }

  // ... with item R of the next step's pixels split and stored between its MFMAs (four VALU instructions per MFMA gap)
#define SESSD_DS_TAPW(T, PAR, R)                                                                    \
  {                                                                                                 \
    SESSD_DS_LOADA(((T) + 2) % 3, s * 9 + (T) + 2)                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    SESSD_DS_MMA((T) % 3, PAR)                                                                      \
    SESSD_DS_SPLITX(R)                                                                              \
    SESSD_DS_STOREX(voff ^ XBUF, R)                                                                 \
    _Pragma("unroll") for (int g = 0; g < 12; ++g) {                                                \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                            \
      __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);                                            \
    }                                                                                               \
    __builtin_amdgcn_sched_group_barrier(0x200, 3, 0);                                              \
    __builtin_amdgcn_sched_barrier(0);                                                              \
  }
  // plane P of the B fragments of e group E
#define SESSD_DS_READBP(VOFF, E, P)                                                                 \
  {                                                                                                 \
    _Pragma("unroll") for (int q = 0; q < 2; ++q)                                                   \
      bf[q][P] = __builtin_bit_cast(bf16x8, *static_cast<const u32x4g*>(__builtin_assume_aligned(    \
          lds + (VOFF) + rthr + (((E)*NPB + q) * 3 + (P)) * 256, 16)));                               \
  }
  // the last tap of an e group: every plane of the NEXT group's B fragments is read as soon as its last use has issued
#define SESSD_DS_TAPR(T, PAR, ENEXT)                                                                \
  {                                                                                                 \
    SESSD_DS_LOADA(((T) + 2) % 3, s * 9 + (T) + 2)                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    SESSD_DS_M((T) % 3, PAR, 2, 0)                                                                  \
    SESSD_DS_M((T) % 3, PAR, 1, 1)                                                                  \
    SESSD_DS_M((T) % 3, PAR, 0, 2)                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    SESSD_DS_READBP(voff, ENEXT, 2)                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    SESSD_DS_M((T) % 3, PAR, 1, 0)                                                                  \
    SESSD_DS_M((T) % 3, PAR, 0, 1)                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    SESSD_DS_READBP(voff, ENEXT, 1)                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    SESSD_DS_M((T) % 3, PAR, 0, 0)                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    SESSD_DS_READBP(voff, ENEXT, 0)                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                              \
  }

  SESSD_DS_LOADX(0)
  SESSD_DS_LOADA(0, 0)
  SESSD_DS_LOADA(1, 1)
  __builtin_amdgcn_sched_barrier(0);
  SESSD_DS_SPLITX(0)
  SESSD_DS_STOREX(0, 0)
  SESSD_DS_SPLITX(1)
  SESSD_DS_STOREX(0, 1)
  SESSD_LDS_BARRIER();
  int voff = 0;
  for (int s = 0; s < KS; ++s) {
    SESSD_DS_LOADX(min(s + 1, KS - 1))
    SESSD_DS_READB(voff, 0)
    __builtin_amdgcn_sched_barrier(0);
    SESSD_DS_TAP(0, 0)   // W11 X00
    SESSD_DS_TAP(1, 1)   // W12 X00
    SESSD_DS_TAP(2, 2)   // W21 X00
    // W22 X00, then W10 X01 (the other buffer was last read in step s - 1, behind the barrier that ended it: it may be written
    // anywhere in step s; at the last step the clamped loads are split once more and nobody reads them)
    SESSD_DS_TAPR(3, 3, 1)
    SESSD_DS_TAPW(4, 1, 0)
    // W20 X01, then W01 X10
    SESSD_DS_TAPR(5, 3, 2)
    SESSD_DS_TAPW(6, 2, 1)
    // W02 X10, then W00 X11
    SESSD_DS_TAPR(7, 3, 3)
    SESSD_DS_TAP(8, 3)
    SESSD_LDS_BARRIER();
    voff ^= XBUF;
  }
#undef SESSD_DS_LOADX
#undef SESSD_DS_LOADA
#undef SESSD_DS_READB
#undef SESSD_DS_M
#undef SESSD_DS_MMA
#undef SESSD_DS_TAP
#undef SESSD_DS_TAPW
#undef SESSD_DS_TAPR
#undef SESSD_DS_READBP
#undef SESSD_DS_SPLITX
#undef SESSD_DS_STOREX

  // ---- epilogue, as dense_deconv_pair.hip: D column = lane & 31 (pixel), row = (r & 3) + 8 (r >> 2) + 4 h (cout); an element
  // past the count or beyond cout gets an out-of-range buffer offset
  const unsigned oplane = 4u * (unsigned)npix;   // output plane in floats
  const unsigned obytes = (unsigned)A.batch * A.cout * oplane * 4u;
  const float* res = A.residual[layer];
  const float* scale = A.scale[layer];
  const float* shift = A.shift[layer];
  const rsrc_t orr = make_rsrc(A.out[layer], obytes);
  const rsrc_t rr = make_rsrc(res ? res : A.out[layer], res ? obytes : 0u);
  const rsrc_t scr = make_rsrc(scale ? scale : A.in, scale ? (unsigned)A.cout * 4u : 0u);
  const rsrc_t shr = make_rsrc(shift ? shift : A.in, shift ? (unsigned)A.cout * 4u : 0u);
  const int co0 = grp * 128 + cb * 32 + 4 * h;
  float scv[16], shv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int k = (r & 3) + 8 * (r >> 2);
    scv[r] = scale ? bufload(scr, (unsigned)(co0 + k) * 4u, 0) : 1.f;
    shv[r] = bufload(shr, (unsigned)(co0 + k) * 4u, 0);
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    int img, y0, x0;
    const bool live = tile_of(A, n_list, unit * NE + (2 * ph + q) * 8 + (j >> 2), img, y0, x0);
    const int y = y0 + ((j >> 1) & 1), x = x0 + (j & 1);
#pragma unroll
    for (int py = 0; py < 2; ++py) {
      const unsigned vbase = ((unsigned)(img * A.cout + co0) * oplane + (unsigned)((2 * y + py) * (2 * A.win) + 2 * x)) * 4u;
      unsigned vo[16];
      f32x2v rv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = (r & 3) + 8 * (r >> 2);
        vo[r] = (live && co0 + k < A.cout) ? vbase + (unsigned)k * oplane * 4u : SESSD_OOB;
        rv[r] = __builtin_bit_cast(f32x2v, __builtin_amdgcn_raw_buffer_load_b64(rr, (int)vo[r], 0, 0));
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v0 = fmaf(acc[2 * py][q][r], scv[r], shv[r]), v1 = fmaf(acc[2 * py + 1][q][r], scv[r], shv[r]);
        if (A.relu) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); }
        f32x2v v;
        v.x = res ? v0 + rv[r].x : v0;
        v.y = res ? v1 + rv[r].y : v1;
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2g, v), orr, (int)vo[r], 0, 0);
      }
    }
  }
}

// bytes of one layer's split weight planes
size_t split_pack_bytes(int cin, int cout) { return (size_t)sessd_divup(cout, 128) * (cin / 16) * 27 * 4096; }

}  // namespace

extern "C" {

// The two ConvTranspose2d(cin, cout, 3, 2, 1, 1) layers of sessd_deconv2d_s2_mfma_pair over the same tile list, on the
// bf16 matrix cores with three-way split operands (f32 accuracy). wsplit_a / wsplit_b: each layer's weight as three bf16 planes
// in fragment order (ops.pack_deconv2d_s2(w).wsplit(): ceil(cout / 128) * cin / 16 * 27 * 4096 bytes); the tap tables are
// the fixed ones of a stride-2 3x3 transposed conv. cin % 16 == 0, even hin / win, the whole batch inside 32-bit offsets.
// One workgroup of 4 waves per (16 list entries, 128 couts, layer), two per CU; no scratch (resources in the header above).
int sessd_deconv2d_s2_pair_split_active(const float* in, int batch, int cin, int hin, int win, const void* wsplit_a, const void* wsplit_b,
                                        float* out_a, float* out_b, int cout, const sessd_conv_epilogue_t* epilogue_a,
                                        const sessd_conv_epilogue_t* epilogue_b, const sessd_tile_list_t* list, hipStream_t stream) {
  if (cin < 16 || cin % 16 || batch < 1 || cout < 1 || hin < 2 || win < 2 || (hin & 1) || (win & 1)) return SESSD_EINVAL;
  if (!in || !wsplit_a || !wsplit_b || !out_a || !out_b || !list || !sessd_tile_list_ok(list)) return SESSD_EINVAL;
  if ((long long)batch * cout * 4 * hin * win * 4 >= 0x7fffffffLL || (long long)batch * cin * hin * win * 4 >= 0x7fffffffLL) return SESSD_EINVAL;
  if (split_pack_bytes(cin, cout) >= 0x7fffffffULL) return SESSD_EINVAL;
  const sessd_conv_epilogue_t none = {nullptr, nullptr, nullptr, 0};
  const sessd_conv_epilogue_t* e[2] = {epilogue_a ? epilogue_a : &none, epilogue_b ? epilogue_b : &none};
  if ((e[0]->relu != 0) != (e[1]->relu != 0)) return SESSD_EINVAL;   // the kernel has one activation for both layers
  DeconvSplitArgs A;
  A.in = in; A.w[0] = wsplit_a; A.w[1] = wsplit_b; A.out[0] = out_a; A.out[1] = out_b;
  for (int l = 0; l < 2; ++l) { A.scale[l] = e[l]->scale; A.shift[l] = e[l]->shift; A.residual[l] = e[l]->residual; }
  sessd_take_tile_list(A, list);
  A.batch = batch; A.cin = cin; A.hin = hin; A.win = win; A.cout = cout; A.relu = e[0]->relu; A.ngroups = sessd_divup(cout, 128);
  const long long wgs = (long long)sessd_divup(list->cap, 16) * A.ngroups * 2;
  if (wgs > 0x7fffffffLL) return SESSD_EINVAL;
  SESSD_LAUNCH(deconv_pair_split_kernel<4>, dim3((unsigned)wgs), dim3(256), 0, stream, A);
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}

}  // extern "C"
