// PointPillars front end: PillarFeatureNet.forward with ONE PFNLayer in eval mode + PointPillarsScatter.forward
// (det3d/models/readers/pillar_encoder.py:114-153 and :173-208) in one launch.
//
// One wave per pillar, lane = output channel (C = 64). A lane keeps its K = 9 / 10 weights and the folded BatchNorm1d in
// registers. The pillar's LIVE points are loaded one per lane as float4, 64 per round (the padding slots of the (N, T, 4)
// tensor are never read: mean KITTI pillars hold a few points out of T = 100); the wave sums x, y, z for the mean; every point's
// four values then reach all lanes through v_readlane (the point index is wave-uniform) and each lane runs its FMA chain,
// the affine, the ReLU and a running max. What the reference computes for the padding slots -- all K columns times 0, so
// relu(shift[c]) -- enters the max arithmetically when num_points < T. The feature row is one coalesced 256-byte store; the
// canvas column (frame b, cell y * nx + x) is 64 stores a plane apart, scattered by nature.
//
// sessd_pillar_frames runs the same arithmetic (pillar_wave_max) straight from the staged clouds: the voxelizer's insert, count and
// assign launches (sessd_voxelize_front, voxelize.hip), then pillar_frames_kernel, one wave per pillar and one grid row per frame,
// which reads the pillar's ascending point-index list 64 entries per round and loads the live points itself -- no (N, T, 4) tensor.
//
// Built with -ffp-contract=off: the centre columns -(float(coor) * v + offset) round as the reference's two operations do. The
// dot product is an explicit fmaf chain.
#include "common.hpp"

namespace {

constexpr int PIL_C = 64;        // output channels = lanes of a wave
constexpr int PIL_WAVES = 4;     // pillars in flight per workgroup
constexpr int PIL_MAX_BLOCKS = 2048;

struct PillarArgs {
  const float4* voxels;          // (N_cap, T) float4
  const int* num_points;
  const int* coors;              // (N_cap, 4) [b, z, y, x]
  const int* n_dev;
  int n_host, T;
  float vx, vy, xo, yo;
  const float* w;                // (64, K)
  const float* scale;
  const float* shift;
  int batch, ny, nx;
  float* feat;                   // (N_cap, 64) or null
  float* canvas;                 // (batch, 64, ny, nx) or null
  int* err;                      // null or one word: set to 1 when a pillar's cell is outside the canvas
};

static __device__ __forceinline__ float lane_bcast(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

static __device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// canvas column of one pillar: nothing is stored for a cell outside (batch, ny, nx)
static __device__ __forceinline__ void store_cell(const PillarArgs& A, int lane, int b, int y, int x, float m) {
  if ((unsigned)b < (unsigned)A.batch && (unsigned)y < (unsigned)A.ny && (unsigned)x < (unsigned)A.nx) {
    A.canvas[(((size_t)b * PIL_C + lane) * A.ny + y) * A.nx + x] = m;
  } else if (A.err != nullptr && lane == 0) {
    A.err[0] = 1;
  }
}

// One pillar's 64 outputs, one per lane: the mean of its np live points, the K-column dot product per point, the folded
// BatchNorm, the ReLU and the max over the T slots. load(slot) returns the point in live slot `slot` (< np) as [x, y, z, r]. The ONE
// copy of this arithmetic: pillar_features_kernel reads the (N, T, 4) tensor through it, pillar_frames_kernel the staged cloud
// through the voxelizer's index lists, and the two must agree bit for bit.
//
// The pieces are shared with the train-mode kernels below, which must form the same bits: pillar_frame (the mean and the centre
// columns), pillar_dist (the distance column) and the visitor -- visit(slot, z, val) sees every live slot's Linear output z and its
// value val = z * sc + sh before the ReLU, in slot order.
struct PillarFrame { float mx, my, mz, fcx, fcy; };   // the per-pillar constants of the decorated row

static __device__ __forceinline__ float pillar_dist(float px, float py, float pz) { return __fsqrt_rn(px * px + py * py + pz * pz); }

// pass 1: the mean of the live points; returns round 0's point of this lane (zeros for lane >= np)
template <class Load>
static __device__ __forceinline__ float4 pillar_frame(int lane, int np, int x, int y, float vx, float vy, float xo, float yo, Load load,
                                                      PillarFrame& F) {
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 p0 = lane < np ? load(lane) : zero4;
  float sx = p0.x, sy = p0.y, sz = p0.z;
  for (int base = 64; base < np; base += 64) {
    const float4 p = base + lane < np ? load(base + lane) : zero4;
    sx += p.x; sy += p.y; sz += p.z;
  }
  const float fn = (float)np;
  F.mx = __fdiv_rn(wave_sum_f(sx), fn); F.my = __fdiv_rn(wave_sum_f(sy), fn); F.mz = __fdiv_rn(wave_sum_f(sz), fn);
  // the centre columns of this fork: per-pillar constants (pillar_encoder.py:126-133)
  F.fcx = -((float)x * vx + xo);
  F.fcy = -((float)y * vy + yo);
  return p0;
}

template <bool DIST, class Load, class Visit>
static __device__ __forceinline__ float pillar_wave_visit(int lane, int np, int T, int x, int y, float vx, float vy, float xo, float yo,
                                                          const float (&w)[DIST ? 10 : 9], float sc, float sh, Load load,
                                                          PillarFrame& F, Visit visit) {
  constexpr int K = DIST ? 10 : 9;
  const float pad = fmaxf(sh, 0.f);  // a padding slot: every column 0 -> relu(0 * scale + shift)
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 p0 = pillar_frame(lane, np, x, y, vx, vy, xo, yo, load, F);   // (round 0 stays in registers for pass 2)
  const float mx = F.mx, my = F.my, mz = F.mz;
  const float cbase = fmaf(w[8], F.fcy, w[7] * F.fcx);
  // pass 2: per point, the K-column dot product, BatchNorm (folded), ReLU, max
  float m = np < T ? pad : 0.f;    // ReLU outputs are >= 0: 0 is the identity of the max over the live points
  for (int base = 0; base < np; base += 64) {
    const float4 p = base == 0 ? p0 : (base + lane < np ? load(base + lane) : zero4);
    const int cnt = np - base < 64 ? np - base : 64;
    for (int j = 0; j < cnt; ++j) {
      const float px = lane_bcast(p.x, j), py = lane_bcast(p.y, j), pz = lane_bcast(p.z, j), pr = lane_bcast(p.w, j);
      float a = w[0] * px;
      a = fmaf(w[1], py, a);
      a = fmaf(w[2], pz, a);
      a = fmaf(w[3], pr, a);
      a = fmaf(w[4], px - mx, a);
      a = fmaf(w[5], py - my, a);
      a = fmaf(w[6], pz - mz, a);
      a += cbase;
      if (DIST) a = fmaf(w[K - 1], pillar_dist(px, py, pz), a);
      const float val = a * sc + sh;
      visit(base + j, a, val);
      m = fmaxf(m, val);
    }
  }
  return m;
}

template <bool DIST, class Load>
static __device__ __forceinline__ float pillar_wave_max(int lane, int np, int T, int x, int y, float vx, float vy, float xo, float yo,
                                                        const float (&w)[DIST ? 10 : 9], float sc, float sh, Load load) {
  PillarFrame F;
  return pillar_wave_visit<DIST>(lane, np, T, x, y, vx, vy, xo, yo, w, sc, sh, load, F, [](int, float, float) {});
}

template <bool DIST>
__global__ __launch_bounds__(PIL_WAVES * 64) void pillar_features_kernel(PillarArgs A) {
  constexpr int K = DIST ? 10 : 9;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int n = A.n_dev ? A.n_dev[0] : A.n_host;
  n = n < A.n_host ? n : A.n_host;   // never past the capacity the host stated
  float w[K];
#pragma unroll
  for (int k = 0; k < K; ++k) w[k] = A.w[lane * K + k];
  const float sc = A.scale[lane], sh = A.shift[lane];

  for (int v = blockIdx.x * PIL_WAVES + wave; v < n; v += gridDim.x * PIL_WAVES) {
    int np = __builtin_amdgcn_readfirstlane(A.num_points[v]);
    np = np < 0 ? 0 : (np > A.T ? A.T : np);
    const int4 co = *reinterpret_cast<const int4*>(A.coors + (size_t)v * 4);
    const int b = __builtin_amdgcn_readfirstlane(co.x), y = __builtin_amdgcn_readfirstlane(co.z),
              x = __builtin_amdgcn_readfirstlane(co.w);
    const float4* src = A.voxels + (size_t)v * A.T;
    const float m = pillar_wave_max<DIST>(lane, np, A.T, x, y, A.vx, A.vy, A.xo, A.yo, w, sc, sh,
                                          [src](int slot) { return src[slot]; });
    if (A.feat != nullptr) A.feat[(size_t)v * PIL_C + lane] = m;
    if (A.canvas != nullptr) store_cell(A, lane, b, y, x, m);
  }
}

// sessd_pillar_frames: the voxelizer's state in place of the (N, T, 4) tensor. One wave per pillar, blockIdx.y = frame.
struct FrameArgs {
  PillarArgs P;                  // reader arguments and outputs (voxels, n_dev, n_host unused; num_points is an OUTPUT here)
  const float4* points;          // (batch, points_per_frame) staged clouds
  int points_per_frame, max_voxels;
  uint32_t hash_capacity;
  const int* lists;              // (hash_capacity, T) ascending point indices per occupied hash entry
  const int* entry_of_vid;       // (batch, max_voxels)
  const int* meta;               // (batch, 4): [cut, unique cells, -, -]
  const int* prefix;             // (batch + 1)
  int* num_points_out;           // (N_cap) or null
};

template <bool DIST>
__global__ __launch_bounds__(PIL_WAVES * 64) void pillar_frames_kernel(FrameArgs F) {
  constexpr int K = DIST ? 10 : 9;
  const PillarArgs& A = F.P;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = blockIdx.y;
  const int vid = blockIdx.x * PIL_WAVES + wave;
  const int* meta = F.meta + fr * 4;
  const int cut = __builtin_amdgcn_readfirstlane(meta[0]);
  const int uniq = __builtin_amdgcn_readfirstlane(meta[1]);
  if (vid >= (uniq < F.max_voxels ? uniq : F.max_voxels)) return;   // wave-uniform
  const int e = __builtin_amdgcn_readfirstlane(F.entry_of_vid[(size_t)fr * F.max_voxels + vid]);
  if ((uint32_t)e >= F.hash_capacity) return;   // (every voxel id below the count has its entry: never taken)
  const int row = __builtin_amdgcn_readfirstlane(F.prefix[fr]) + vid;
  if ((uint32_t)row >= (uint32_t)A.batch * (uint32_t)F.max_voxels) return;   // (a prefix[0] the caller did not zero: no row to write)
  const int* L = F.lists + (size_t)e * A.T;
  const float4* pts = F.points + (size_t)fr * F.points_per_frame;
  const int P = F.points_per_frame;
  // the live slots: a prefix of the ascending list, those below the cut (the empty marker is never below it)
  const int T = A.T;
  auto live_index = [L, cut, P, T](int slot) {
    const int idx = slot < T ? L[slot] : SESSD_SENT;
    return (idx < cut && (uint32_t)idx < (uint32_t)P) ? idx : -1;
  };
  const int idx0 = live_index(lane);
  int np = __popcll(__ballot(idx0 >= 0));
  for (int base = 64; base < A.T; base += 64) np += __popcll(__ballot(live_index(base + lane) >= 0));
  np = __builtin_amdgcn_readfirstlane(np);
  const int4 co = *reinterpret_cast<const int4*>(A.coors + (size_t)row * 4);
  const int b = __builtin_amdgcn_readfirstlane(co.x), y = __builtin_amdgcn_readfirstlane(co.z),
            x = __builtin_amdgcn_readfirstlane(co.w);
  float w[K];
#pragma unroll
  for (int k = 0; k < K; ++k) w[k] = A.w[lane * K + k];
  const float sc = A.scale[lane], sh = A.shift[lane];
  // load() is called for slots < np only, which are live (round 0: the lane's own slot, its index already in a register)
  const float m = pillar_wave_max<DIST>(lane, np, T, x, y, A.vx, A.vy, A.xo, A.yo, w, sc, sh, [pts, idx0, L, P](int slot) {
    const int idx = slot < 64 ? idx0 : L[slot];
    return pts[(uint32_t)idx < (uint32_t)P ? idx : 0];
  });
  if (F.num_points_out != nullptr && lane == 0) F.num_points_out[row] = np;
  if (A.feat != nullptr) A.feat[(size_t)row * PIL_C + lane] = m;
  store_cell(A, lane, b, y, x, m);
}

// scatter alone: rows of a finished (N_cap, 64) feature tensor onto the canvas
__global__ __launch_bounds__(PIL_WAVES * 64) void pillar_scatter_kernel(PillarArgs A) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int n = A.n_dev ? A.n_dev[0] : A.n_host;
  n = n < A.n_host ? n : A.n_host;
  for (int v = blockIdx.x * PIL_WAVES + wave; v < n; v += gridDim.x * PIL_WAVES) {
    const int4 co = *reinterpret_cast<const int4*>(A.coors + (size_t)v * 4);
    store_cell(A, lane, co.x, co.z, co.w, A.feat[(size_t)v * PIL_C + lane]);
  }
}

// ------------------------------------------------------------------------------------------------ train mode (one PFN layer)
// BatchNorm1d in train mode normalises a channel over ALL M = n * T slots; a padding slot's Linear output is 0. With f_i the
// decorated row of live slot i (formed in float64 from the float32 points: pillar_row_d), S1 = sum f_i and G = sum f_i f_i^T over the live slots, channel c with weight row w_c has
// sum z = w_c . S1 and sum z^2 = w_c^T G w_c: the statistics of all 64 channels follow from K + K (K + 1) / 2 totals that no channel
// owns. The forward output is pillar_features_kernel with scale = gamma * invstd, shift = beta - mean * scale. The backward needs
// the (pillar, channel) pair's selected slot only -- the first slot whose value equals the stored output bit for bit, found by
// running pillar_wave_visit again; the padding candidate (slots >= num_points) comes after every live slot -- and closes the
// BatchNorm's and the Linear's gradients over the totals:
//   dy = g where the selected value is > 0, xhat = (w . f_s - mean) * invstd for a live slot, -mean * invstd for a padding slot
//   dbeta = sum dy, dgamma = sum dy * xhat = invstd * (sum dy z_s - mean * sum dy), P = sum over live selected slots of dy * f_s
//   dW_c = scale_c * [P_c - dbeta_c / M * S1 - dgamma_c / M * invstd_c * (G w_c - mean_c * S1)]
// Totals are float64; every sum has a fixed order (a lane's pillars in row order, the wave's butterfly, the block's waves in
// order, the blocks in order by the blocks that arrive last: pt_final_sum, with bn_train.hip's counter words, zero on entry and
// on return).
constexpr int PT_STATS_BLOCKS = 256;   // x 4 waves (16 groups of PT_GROUP blocks: the counter words fit the 256 bytes)
constexpr int PT_SEL_WAVES = 8;
constexpr int PT_SEL_BLOCKS = 128;
constexpr size_t PT_COUNTER_BYTES = 256;

__host__ __device__ constexpr int pt_ntot(int K) { return K + K * (K + 1) / 2; }          // S1, upper triangle of G by rows (M follows)
__host__ __device__ constexpr int pt_gidx(int K, int a, int b) { return K + a * K - a * (a - 1) / 2 + (b - a); }   // a <= b
__host__ __device__ constexpr int pt_nbwd(int K) { return (2 + K) * PIL_C; }              // sum dy, sum dy * z, P (C, K)

static __device__ __forceinline__ void pt_put(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
static __device__ __forceinline__ double pt_get(const double* p) {
  return __hip_atomic_load(const_cast<double*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static __device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The decorated row in float64, from the float32 points: what the totals and the gradients are made of (the selection alone runs
// the forward's float32 arithmetic). vx, vy and the offsets enter as the float32 values the forward uses.
struct PillarFrameD { double mx, my, mz, fcx, fcy; };

template <class Load>
static __device__ __forceinline__ void pillar_frame_d(int lane, int np, int x, int y, float vx, float vy, float xo, float yo, Load load,
                                                      PillarFrameD& D) {
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int base = 0; base < np; base += 64) {
    if (base + lane < np) {
      const float4 p = load(base + lane);
      sx += (double)p.x; sy += (double)p.y; sz += (double)p.z;
    }
  }
  const double dn = (double)np;   // np = 0: no live slot uses the means
  D.mx = wave_sum_d(sx) / dn; D.my = wave_sum_d(sy) / dn; D.mz = wave_sum_d(sz) / dn;
  D.fcx = -((double)x * (double)vx + (double)xo);
  D.fcy = -((double)y * (double)vy + (double)yo);
}

template <int K>
static __device__ __forceinline__ void pillar_row_d(const float4& p, const PillarFrameD& D, double (&f)[K]) {
  const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
  f[0] = px; f[1] = py; f[2] = pz; f[3] = (double)p.w;
  f[4] = px - D.mx; f[5] = py - D.my; f[6] = pz - D.mz;
  f[7] = D.fcx; f[8] = D.fcy;
  if (K == 10) f[K - 1] = sqrt(px * px + py * py + pz * pz);
}

// The final sum over the blocks, in two levels so that no single block reads every partial from past the L2 (one block alone
// fetches about 65 GB/s there: bn_train.hip). Blocks form groups of PT_GROUP; the block of a group that arrives last adds the
// group's partials in block order into a group partial; the group whose sum is finished last adds the group partials in group
// order into `out`. Both orders are fixed, whichever block arrives last. Nothing waits: a block that is not last leaves.
// counters: word 0 counts finished groups, word 1 + g the arrivals of group g; all zero on entry and zero again on return.
// Every thread of the block calls this after it stored the block's partials (count doubles at partial + blockIdx.x * count);
// gpartial holds divup(gridDim.x, PT_GROUP) * count doubles. Returns true in the block that wrote `out`.
constexpr int PT_GROUP = 16;
static_assert(PT_STATS_BLOCKS <= PT_GROUP * PT_GROUP && PT_SEL_BLOCKS <= PT_GROUP * PT_GROUP, "the group partials are one row-order sum");
static_assert((1 + PT_GROUP) * sizeof(unsigned) <= PT_COUNTER_BYTES, "one counter word per group and one for the groups");

static __device__ __forceinline__ bool pt_count_in(unsigned* word, unsigned expected, int* s_flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this thread's partials are acknowledged
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool last = __hip_atomic_fetch_add(word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == expected - 1;
    if (last) __hip_atomic_store(word, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // everyone expected has arrived
    *s_flag = last ? 1 : 0;
  }
  __syncthreads();
  return *s_flag != 0;
}

// rows [first, first + rows) of src (rows <= PT_GROUP), element j of each, added in row order (all loads in flight at once)
static __device__ __forceinline__ double pt_row_order_sum(const double* src, int first, int rows, int count, int j) {
  double a[PT_GROUP];
#pragma unroll
  for (int k = 0; k < PT_GROUP; ++k) a[k] = k < rows ? pt_get(src + (size_t)(first + k) * count + j) : 0.0;
  double t = 0.0;
#pragma unroll
  for (int k = 0; k < PT_GROUP; ++k) t += a[k];
  return t;
}

static __device__ __forceinline__ bool pt_final_sum(const double* partial, double* gpartial, unsigned* counters, int count, double* out,
                                                    int* s_flag) {
  const int nb = (int)gridDim.x, grp = (int)blockIdx.x / PT_GROUP, ngrp = sessd_divup(nb, PT_GROUP);
  const int first = grp * PT_GROUP, rows = nb - first < PT_GROUP ? nb - first : PT_GROUP;
  if (!pt_count_in(counters + 1 + grp, (unsigned)rows, s_flag)) return false;
  for (int j = threadIdx.x; j < count; j += blockDim.x) pt_put(gpartial + (size_t)grp * count + j, pt_row_order_sum(partial, first, rows, count, j));
  if (!pt_count_in(counters, (unsigned)ngrp, s_flag)) return false;
  for (int j = threadIdx.x; j < count; j += blockDim.x) out[j] = pt_row_order_sum(gpartial, 0, ngrp, count, j);
  return true;
}

// One wave per pillar, lane = live point: S1 and G of the first n pillars -> totals [S1 (K), G upper triangle, M = n * T]
template <bool DIST>
__global__ __launch_bounds__(PIL_WAVES * 64) void pillar_train_stats_kernel(PillarArgs A, double* partial, double* gpartial,
                                                                            unsigned* counters, double* totals) {
  constexpr int K = DIST ? 10 : 9;
  constexpr int NTOT = pt_ntot(K);
  __shared__ double sm[PIL_WAVES][NTOT];
  __shared__ int s_last;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int n = A.n_dev ? A.n_dev[0] : A.n_host;
  n = n < A.n_host ? n : A.n_host;
  n = n < 0 ? 0 : n;
  double acc[NTOT];
#pragma unroll
  for (int t = 0; t < NTOT; ++t) acc[t] = 0.0;
  for (int v = blockIdx.x * PIL_WAVES + wave; v < n; v += gridDim.x * PIL_WAVES) {
    int np = __builtin_amdgcn_readfirstlane(A.num_points[v]);
    np = np < 0 ? 0 : (np > A.T ? A.T : np);
    const int4 co = *reinterpret_cast<const int4*>(A.coors + (size_t)v * 4);
    const int y = __builtin_amdgcn_readfirstlane(co.z), x = __builtin_amdgcn_readfirstlane(co.w);
    const float4* src = A.voxels + (size_t)v * A.T;
    auto load = [src](int slot) { return src[slot]; };
    PillarFrameD D;
    pillar_frame_d(lane, np, x, y, A.vx, A.vy, A.xo, A.yo, load, D);
    for (int base = 0; base < np; base += 64) {
      if (base + lane < np) {
        double f[K];
        pillar_row_d<K>(load(base + lane), D, f);
#pragma unroll
        for (int a = 0; a < K; ++a) {
          acc[a] += f[a];
#pragma unroll
          for (int b = a; b < K; ++b) acc[pt_gidx(K, a, b)] += f[a] * f[b];
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NTOT; ++t) {
    const double s = wave_sum_d(acc[t]);
    if (lane == 0) sm[wave][t] = s;
  }
  __syncthreads();
  if (threadIdx.x < NTOT) {
    double s = sm[0][threadIdx.x];
    for (int wv = 1; wv < PIL_WAVES; ++wv) s += sm[wv][threadIdx.x];
    pt_put(partial + (size_t)blockIdx.x * NTOT + threadIdx.x, s);
  }
  if (!pt_final_sum(partial, gpartial, counters, NTOT, totals, &s_last)) return;
  if (threadIdx.x == 0) totals[NTOT] = (double)n * (double)A.T;
}

// One channel's batch statistics from the totals: sum z = w . S1, sum z^2 = w^T G w over M = n rows
template <int K>
static __device__ __forceinline__ void pt_channel_stats(const double* __restrict__ totals, const double (&wc)[K], float eps, double& n,
                                                        double& m, double& var, double& r) {
  double sz = 0.0, szz = 0.0;
#pragma unroll
  for (int a = 0; a < K; ++a) {
    sz += wc[a] * totals[a];
    szz += wc[a] * wc[a] * totals[pt_gidx(K, a, a)];
#pragma unroll
    for (int b = a + 1; b < K; ++b) szz += 2.0 * wc[a] * wc[b] * totals[pt_gidx(K, a, b)];
  }
  n = totals[pt_ntot(K)];
  m = n > 0 ? sz / n : 0.0;
  var = n > 0 ? szz / n - m * m : 0.0;
  if (var < 0.0) var = 0.0;
  r = 1.0 / sqrt(var + (double)eps);
}

// totals (of all ranks) -> mean, invstd, the folded scale / shift, the running statistics; lane = channel. The row count's
// edge cases are sessd_bn_relu_train_apply's: M = 0 gives mean 0, variance 0 and leaves the running statistics alone, M = 1 puts
// the biased variance into running_var.
template <int K>
__global__ __launch_bounds__(PIL_C) void pillar_train_finalize_kernel(const double* __restrict__ totals, const float* __restrict__ w,
                                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                      float eps, float momentum, float* running_mean,
                                                                      float* running_var, float* mean, float* invstd, float* scale,
                                                                      float* shift) {
  const int c = threadIdx.x;
  double wc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) wc[k] = (double)w[c * K + k];
  double n, m, var, r;
  pt_channel_stats<K>(totals, wc, eps, n, m, var, r);
  mean[c] = (float)m;
  invstd[c] = (float)r;
  const double s = (double)gamma[c] * r;
  scale[c] = (float)s;
  shift[c] = (float)((double)beta[c] - m * s);
  if (running_mean && n > 0) {
    const double unbiased = n > 1 ? var * n / (n - 1) : var;
    running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * m);
    running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * unbiased);
  }
}

struct PillarSelectArgs {
  const float* out;              // (N_cap, 64) the forward output
  const float* grad;             // (N_cap, 64) its gradient
  double* partial;
  double* gpartial;
  unsigned* counters;
  double* totals;                // [sum dy (64), sum dy * z (64), P (64, K)]
};

// One wave per pillar, lane = channel: the selected slot by recomputation, dy, and the sums over the first n pillars
template <bool DIST>
__global__ __launch_bounds__(PT_SEL_WAVES * 64) void pillar_train_select_kernel(PillarArgs A, PillarSelectArgs S) {
  constexpr int K = DIST ? 10 : 9;
  constexpr int NB = pt_nbwd(K);
  __shared__ double sm[PT_SEL_WAVES][NB];
  __shared__ int s_last;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int n = A.n_dev ? A.n_dev[0] : A.n_host;
  n = n < A.n_host ? n : A.n_host;
  float w[K];
#pragma unroll
  for (int k = 0; k < K; ++k) w[k] = A.w[lane * K + k];
  const float sc = A.scale[lane], sh = A.shift[lane];
  double db = 0.0, dz = 0.0, P[K];   // sum dy, sum dy * z (z = 0 in a padding slot), sum dy * f
#pragma unroll
  for (int k = 0; k < K; ++k) P[k] = 0.0;
  for (int v = blockIdx.x * PT_SEL_WAVES + wave; v < n; v += gridDim.x * PT_SEL_WAVES) {
    int np = __builtin_amdgcn_readfirstlane(A.num_points[v]);
    np = np < 0 ? 0 : (np > A.T ? A.T : np);
    const int4 co = *reinterpret_cast<const int4*>(A.coors + (size_t)v * 4);
    const int y = __builtin_amdgcn_readfirstlane(co.z), x = __builtin_amdgcn_readfirstlane(co.w);
    const float4* src = A.voxels + (size_t)v * A.T;
    const float out = S.out[(size_t)v * PIL_C + lane];
    const double g = (double)S.grad[(size_t)v * PIL_C + lane];
    int sel = -1;
    auto load = [src](int slot) { return src[slot]; };
    PillarFrame F;
    pillar_wave_visit<DIST>(lane, np, A.T, x, y, A.vx, A.vy, A.xo, A.yo, w, sc, sh, load, F, [&sel, out](int slot, float, float val) {
      if (sel < 0 && val == out) sel = slot;
    });
    PillarFrameD D;
    pillar_frame_d(lane, np, x, y, A.vx, A.vy, A.xo, A.yo, load, D);
    if (!(out > 0.f)) {                  // clamped by the ReLU (or a maximum of exactly 0): no gradient
    } else if (sel >= 0) {               // a live slot (sel < np): its row and its Linear output in float64
      double f[K], z = 0.0;
      pillar_row_d<K>(src[sel], D, f);
#pragma unroll
      for (int k = 0; k < K; ++k) z += (double)w[k] * f[k];
      db += g;
      dz += g * z;
#pragma unroll
      for (int k = 0; k < K; ++k) P[k] += g * f[k];
    } else if (np < A.T && sh == out) {  // the padding candidate: z = 0, no row
      db += g;
    }
  }
  sm[wave][lane] = db;
  sm[wave][PIL_C + lane] = dz;
#pragma unroll
  for (int k = 0; k < K; ++k) sm[wave][(2 + k) * PIL_C + lane] = P[k];
  __syncthreads();
  for (int j = threadIdx.x; j < NB; j += PT_SEL_WAVES * 64) {
    // totals' order: sum dy, sum dy * z, then P as (channel, column)
    const int q = j < 2 * PIL_C ? j : (2 + (j - 2 * PIL_C) % K) * PIL_C + (j - 2 * PIL_C) / K;
    double s = sm[0][q];
    for (int wv = 1; wv < PT_SEL_WAVES; ++wv) s += sm[wv][q];
    pt_put(S.partial + (size_t)blockIdx.x * NB + j, s);
  }
  pt_final_sum(S.partial, S.gpartial, S.counters, NB, S.totals, &s_last);
}

// lane = channel. bwd / fwd: this rank's totals (P, S1, G); bwd_all / fwd_all: those of all ranks (the sums of dy and dy * z, M).
// mean, invstd and scale are recomputed in float64 from fwd_all: dgamma = invstd * (sum dy z - mean * sum dy).
template <int K>
__global__ __launch_bounds__(PIL_C) void pillar_train_bwd_finalize_kernel(const double* __restrict__ bwd, const double* __restrict__ bwd_all,
                                                                          const double* __restrict__ fwd, const double* __restrict__ fwd_all,
                                                                          const float* __restrict__ w, const float* __restrict__ gamma,
                                                                          float eps, float* dw, float* dgamma, float* dbeta) {
  const int c = threadIdx.x;
  double wc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) wc[k] = (double)w[c * K + k];
  double M, mu, var, r;
  pt_channel_stats<K>(fwd_all, wc, eps, M, mu, var, r);
  const double s = (double)gamma[c] * r;
  const double inv_m = M > 0 ? 1.0 / M : 0.0;
  const double kb = bwd_all[c] * inv_m;
  const double kg = r * (bwd_all[PIL_C + c] - mu * bwd_all[c]) * inv_m * r;   // dgamma of all ranks / M * invstd
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double gw = 0.0;
#pragma unroll
    for (int l = 0; l < K; ++l) gw += fwd[k <= l ? pt_gidx(K, k, l) : pt_gidx(K, l, k)] * wc[l];
    dw[c * K + k] = (float)(s * (bwd[2 * PIL_C + c * K + k] - kb * fwd[k] - kg * (gw - mu * fwd[k])));
  }
  dgamma[c] = (float)(r * (bwd[PIL_C + c] - mu * bwd[c]));
  dbeta[c] = (float)bwd[c];
}

// The scatter's gradient: one wave per row, lane = channel; rows >= n and pillars whose cell is outside the canvas get zeros
__global__ __launch_bounds__(PIL_WAVES * 64) void pillar_scatter_bwd_kernel(const float* __restrict__ grad_canvas,
                                                                            const int* __restrict__ coors, const int* n_dev,
                                                                            int n_host, int batch, int ny, int nx,
                                                                            float* __restrict__ grad_feat) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int n = n_dev ? n_dev[0] : n_host;
  n = n < n_host ? n : n_host;
  for (int v = blockIdx.x * PIL_WAVES + wave; v < n_host; v += gridDim.x * PIL_WAVES) {
    float g = 0.f;
    if (v < n) {
      const int4 co = *reinterpret_cast<const int4*>(coors + (size_t)v * 4);
      const int b = co.x, y = co.z, x = co.w;
      if ((unsigned)b < (unsigned)batch && (unsigned)y < (unsigned)ny && (unsigned)x < (unsigned)nx)
        g = grad_canvas[(((size_t)b * PIL_C + lane) * ny + y) * nx + x];
    }
    grad_feat[(size_t)v * PIL_C + lane] = g;
  }
}

}  // namespace

extern "C" int sessd_pillar_features(const float* voxels, const int* num_points, const int* coors, const int* num_voxels_dev,
                                     int num_voxels_host, int max_points_per_voxel, int ndim, float vx, float vy, float x_offset,
                                     float y_offset, const float* weight, const float* scale, const float* shift, int channels,
                                     int with_distance, int batch, int ny, int nx, float* feat, float* canvas, int* err_flag,
                                     hipStream_t stream) {
  if (ndim != 4 || channels != PIL_C || max_points_per_voxel < 1 || num_voxels_host < 0) return SESSD_EINVAL;
  if (num_voxels_host == 0) return SESSD_OK;  // nothing to do (an empty tensor's pointer may well be null)
  if (feat == nullptr && canvas == nullptr) return SESSD_EINVAL;
  if (coors == nullptr) return SESSD_EINVAL;
  if (canvas != nullptr && (batch < 1 || ny < 1 || nx < 1)) return SESSD_EINVAL;
  const bool scatter_only = voxels == nullptr;
  if (scatter_only) {
    if (feat == nullptr || canvas == nullptr) return SESSD_EINVAL;
  } else if (num_points == nullptr || weight == nullptr || scale == nullptr || shift == nullptr) {
    return SESSD_EINVAL;
  }
  PillarArgs A;
  A.voxels = reinterpret_cast<const float4*>(voxels);
  A.num_points = num_points; A.coors = coors; A.n_dev = num_voxels_dev; A.n_host = num_voxels_host;
  A.T = max_points_per_voxel;
  A.vx = vx; A.vy = vy; A.xo = x_offset; A.yo = y_offset;
  A.w = weight; A.scale = scale; A.shift = shift;
  A.batch = batch; A.ny = ny; A.nx = nx;
  A.feat = feat; A.canvas = canvas; A.err = err_flag;
  int blocks = sessd_divup(num_voxels_host, PIL_WAVES);
  if (blocks > PIL_MAX_BLOCKS) blocks = PIL_MAX_BLOCKS;
  if (scatter_only)
    SESSD_LAUNCH(pillar_scatter_kernel, dim3(blocks), dim3(PIL_WAVES * 64), 0, stream, A);
  else if (with_distance)
    SESSD_LAUNCH(pillar_features_kernel<true>, dim3(blocks), dim3(PIL_WAVES * 64), 0, stream, A);
  else
    SESSD_LAUNCH(pillar_features_kernel<false>, dim3(blocks), dim3(PIL_WAVES * 64), 0, stream, A);
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}

extern "C" int sessd_pillar_frames(const float* points, int batch, int points_per_frame, int ndim, const float* range6,
                                   const float* voxel_size3, const int* grid3, int max_points_per_voxel, int max_voxels,
                                   uint32_t* hash_keys, int* hash_vals, uint32_t hash_capacity, float vx, float vy, float x_offset,
                                   float y_offset, const float* weight, const float* scale, const float* shift, int channels,
                                   int with_distance, int ny, int nx, float* canvas, int* coors, int* prefix, int* num_points,
                                   float* feat, int* err_flag, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (ndim != 4 || channels != PIL_C || batch < 1 || ny < 1 || nx < 1) return SESSD_EINVAL;
  if (points == nullptr || range6 == nullptr || voxel_size3 == nullptr || grid3 == nullptr || hash_keys == nullptr ||
      hash_vals == nullptr || weight == nullptr || scale == nullptr || shift == nullptr || canvas == nullptr || coors == nullptr ||
      prefix == nullptr || workspace == nullptr)
    return SESSD_EINVAL;
  // the shared launches check the rest (sizes, hash capacity a power of two and >= 2 * batch * points_per_frame, the workspace)
  // before they launch anything
  SessdVoxState st;
  const int rc = sessd_voxelize_front(points, batch, points_per_frame, ndim, range6, voxel_size3, grid3, max_points_per_voxel,
                                      max_voxels, hash_keys, hash_vals, hash_capacity, coors, 4, prefix, workspace, workspace_bytes,
                                      stream, &st);
  if (rc != SESSD_OK) return rc;
  FrameArgs F;
  PillarArgs& A = F.P;
  A.voxels = nullptr; A.num_points = nullptr; A.coors = coors; A.n_dev = nullptr; A.n_host = 0;
  A.T = max_points_per_voxel;
  A.vx = vx; A.vy = vy; A.xo = x_offset; A.yo = y_offset;
  A.w = weight; A.scale = scale; A.shift = shift;
  A.batch = batch; A.ny = ny; A.nx = nx;
  A.feat = feat; A.canvas = canvas; A.err = err_flag;
  F.points = reinterpret_cast<const float4*>(points);
  F.points_per_frame = points_per_frame; F.max_voxels = max_voxels; F.hash_capacity = hash_capacity;
  F.lists = st.lists; F.entry_of_vid = st.entry_of_vid; F.meta = st.meta; F.prefix = prefix;
  F.num_points_out = num_points;
  // the pillar count is on the device: the grid covers what a frame can hold, waves past the count leave at once
  const int blocks = sessd_divup(max_voxels < points_per_frame ? max_voxels : points_per_frame, PIL_WAVES);
  if (with_distance)
    SESSD_LAUNCH(pillar_frames_kernel<true>, dim3(blocks, batch), dim3(PIL_WAVES * 64), 0, stream, F);
  else
    SESSD_LAUNCH(pillar_frames_kernel<false>, dim3(blocks, batch), dim3(PIL_WAVES * 64), 0, stream, F);
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}

// ------------------------------------------------------------------------------------------------ train mode: entry points
namespace {

bool pt_shape_ok(int ndim, int channels, int num_columns, int with_distance) {
  return ndim == 4 && channels == PIL_C && num_columns == (with_distance ? 10 : 9);
}

PillarArgs pt_args(const float* voxels, const int* num_points, const int* coors, const int* n_dev, int n_host, int T, float vx, float vy,
                   float xo, float yo, const float* w, const float* scale, const float* shift) {
  PillarArgs A;
  A.voxels = reinterpret_cast<const float4*>(voxels);
  A.num_points = num_points; A.coors = coors; A.n_dev = n_dev; A.n_host = n_host; A.T = T;
  A.vx = vx; A.vy = vy; A.xo = xo; A.yo = yo;
  A.w = w; A.scale = scale; A.shift = shift;
  A.batch = 0; A.ny = 0; A.nx = 0;
  A.feat = nullptr; A.canvas = nullptr; A.err = nullptr;
  return A;
}

int pt_stats_blocks(int n) { const int b = sessd_divup(n, PIL_WAVES); return b > PT_STATS_BLOCKS ? PT_STATS_BLOCKS : b; }
int pt_select_blocks(int n) { const int b = sessd_divup(n, PT_SEL_WAVES); return b > PT_SEL_BLOCKS ? PT_SEL_BLOCKS : b; }

}  // namespace

extern "C" size_t sessd_pillar_train_totals(int with_distance) { return (size_t)pt_ntot(with_distance ? 10 : 9) + 1; }

extern "C" size_t sessd_pillar_train_bwd_totals(int with_distance) { return (size_t)pt_nbwd(with_distance ? 10 : 9); }

extern "C" size_t sessd_pillar_train_workspace_bytes(int with_distance) {
  const int K = with_distance ? 10 : 9;
  // the blocks' partials and the groups' partials of the larger of the two launches
  const size_t fwd = (size_t)(PT_STATS_BLOCKS + PT_STATS_BLOCKS / PT_GROUP) * pt_ntot(K);
  const size_t bwd = (size_t)(PT_SEL_BLOCKS + PT_SEL_BLOCKS / PT_GROUP) * pt_nbwd(K);
  return PT_COUNTER_BYTES + (fwd > bwd ? fwd : bwd) * sizeof(double);
}

extern "C" int sessd_pillar_train_stats(const float* voxels, const int* num_points, const int* coors, const int* num_voxels_dev,
                                        int num_voxels_host, int max_points_per_voxel, int ndim, float vx, float vy, float x_offset,
                                        float y_offset, int channels, int num_columns, int with_distance, double* totals,
                                        void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!pt_shape_ok(ndim, channels, num_columns, with_distance) || max_points_per_voxel < 1 || num_voxels_host < 1) return SESSD_EINVAL;
  if (voxels == nullptr || num_points == nullptr || coors == nullptr || totals == nullptr || workspace == nullptr) return SESSD_EINVAL;
  if (workspace_bytes < sessd_pillar_train_workspace_bytes(with_distance)) return SESSD_EINVAL;
  const PillarArgs A = pt_args(voxels, num_points, coors, num_voxels_dev, num_voxels_host, max_points_per_voxel, vx, vy, x_offset,
                               y_offset, nullptr, nullptr, nullptr);
  unsigned* counters = (unsigned*)workspace;
  double* partial = (double*)((char*)workspace + PT_COUNTER_BYTES);
  double* gpartial = partial + (size_t)PT_STATS_BLOCKS * pt_ntot(num_columns);
  const int blocks = pt_stats_blocks(num_voxels_host);
  if (with_distance)
    SESSD_LAUNCH(pillar_train_stats_kernel<true>, dim3(blocks), dim3(PIL_WAVES * 64), 0, stream, A, partial, gpartial, counters, totals);
  else
    SESSD_LAUNCH(pillar_train_stats_kernel<false>, dim3(blocks), dim3(PIL_WAVES * 64), 0, stream, A, partial, gpartial, counters, totals);
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}

extern "C" int sessd_pillar_train_finalize(const double* totals, const float* weight, const float* gamma, const float* beta, float eps,
                                           float momentum, int channels, int num_columns, int with_distance, float* running_mean,
                                           float* running_var, float* mean, float* invstd, float* scale, float* shift,
                                           hipStream_t stream) {
  if (!pt_shape_ok(4, channels, num_columns, with_distance)) return SESSD_EINVAL;
  if (totals == nullptr || weight == nullptr || gamma == nullptr || beta == nullptr || mean == nullptr || invstd == nullptr ||
      scale == nullptr || shift == nullptr)
    return SESSD_EINVAL;
  if ((running_mean == nullptr) != (running_var == nullptr)) return SESSD_EINVAL;
  if (with_distance)
    SESSD_LAUNCH(pillar_train_finalize_kernel<10>, dim3(1), dim3(PIL_C), 0, stream, totals, weight, gamma, beta, eps, momentum,
                 running_mean, running_var, mean, invstd, scale, shift);
  else
    SESSD_LAUNCH(pillar_train_finalize_kernel<9>, dim3(1), dim3(PIL_C), 0, stream, totals, weight, gamma, beta, eps, momentum,
                 running_mean, running_var, mean, invstd, scale, shift);
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}

extern "C" int sessd_pillar_train_bwd_select(const float* voxels, const int* num_points, const int* coors, const int* num_voxels_dev,
                                             int num_voxels_host, int max_points_per_voxel, int ndim, float vx, float vy,
                                             float x_offset, float y_offset, const float* weight, const float* scale,
                                             const float* shift, int channels, int num_columns, int with_distance,
                                             const float* feat, const float* grad_feat,
                                             double* bwd_totals, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!pt_shape_ok(ndim, channels, num_columns, with_distance) || max_points_per_voxel < 1 || num_voxels_host < 1) return SESSD_EINVAL;
  if (voxels == nullptr || num_points == nullptr || coors == nullptr || weight == nullptr || scale == nullptr || shift == nullptr ||
      feat == nullptr || grad_feat == nullptr || bwd_totals == nullptr || workspace == nullptr)
    return SESSD_EINVAL;
  if (workspace_bytes < sessd_pillar_train_workspace_bytes(with_distance)) return SESSD_EINVAL;
  const PillarArgs A = pt_args(voxels, num_points, coors, num_voxels_dev, num_voxels_host, max_points_per_voxel, vx, vy, x_offset,
                               y_offset, weight, scale, shift);
  PillarSelectArgs S;
  S.out = feat; S.grad = grad_feat;
  S.counters = (unsigned*)workspace;
  S.partial = (double*)((char*)workspace + PT_COUNTER_BYTES);
  S.gpartial = S.partial + (size_t)PT_SEL_BLOCKS * pt_nbwd(num_columns);
  S.totals = bwd_totals;
  const int blocks = pt_select_blocks(num_voxels_host);
  if (with_distance)
    SESSD_LAUNCH(pillar_train_select_kernel<true>, dim3(blocks), dim3(PT_SEL_WAVES * 64), 0, stream, A, S);
  else
    SESSD_LAUNCH(pillar_train_select_kernel<false>, dim3(blocks), dim3(PT_SEL_WAVES * 64), 0, stream, A, S);
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}

extern "C" int sessd_pillar_train_bwd_finalize(const double* bwd_totals, const double* bwd_totals_all, const double* totals,
                                               const double* totals_all, const float* weight, const float* gamma, float eps,
                                               int channels, int num_columns, int with_distance, float* grad_weight,
                                               float* grad_gamma, float* grad_beta, hipStream_t stream) {
  if (!pt_shape_ok(4, channels, num_columns, with_distance)) return SESSD_EINVAL;
  if (bwd_totals == nullptr || bwd_totals_all == nullptr || totals == nullptr || totals_all == nullptr || weight == nullptr ||
      gamma == nullptr || grad_weight == nullptr || grad_gamma == nullptr || grad_beta == nullptr)
    return SESSD_EINVAL;
  if (with_distance)
    SESSD_LAUNCH(pillar_train_bwd_finalize_kernel<10>, dim3(1), dim3(PIL_C), 0, stream, bwd_totals, bwd_totals_all, totals, totals_all,
                 weight, gamma, eps, grad_weight, grad_gamma, grad_beta);
  else
    SESSD_LAUNCH(pillar_train_bwd_finalize_kernel<9>, dim3(1), dim3(PIL_C), 0, stream, bwd_totals, bwd_totals_all, totals, totals_all,
                 weight, gamma, eps, grad_weight, grad_gamma, grad_beta);
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}

extern "C" int sessd_pillar_scatter_bwd(const float* grad_canvas, const int* coors, const int* num_voxels_dev, int num_voxels_host,
                                        int channels, int batch, int ny, int nx, float* grad_feat, hipStream_t stream) {
  if (channels != PIL_C || num_voxels_host < 1 || batch < 1 || ny < 1 || nx < 1) return SESSD_EINVAL;
  if (grad_canvas == nullptr || coors == nullptr || grad_feat == nullptr) return SESSD_EINVAL;
  int blocks = sessd_divup(num_voxels_host, PIL_WAVES);
  if (blocks > PIL_MAX_BLOCKS) blocks = PIL_MAX_BLOCKS;
  SESSD_LAUNCH(pillar_scatter_bwd_kernel, dim3(blocks), dim3(PIL_WAVES * 64), 0, stream, grad_canvas, coors, num_voxels_dev,
               num_voxels_host, batch, ny, nx, grad_feat);
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}
