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
template <bool DIST, class Load>
static __device__ __forceinline__ float pillar_wave_max(int lane, int np, int T, int x, int y, float vx, float vy, float xo, float yo,
                                                        const float (&w)[DIST ? 10 : 9], float sc, float sh, Load load) {
  constexpr int K = DIST ? 10 : 9;
  const float pad = fmaxf(sh, 0.f);  // a padding slot: every column 0 -> relu(0 * scale + shift)
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  // pass 1: the mean of the live points (round 0 stays in registers for pass 2)
  const float4 p0 = lane < np ? load(lane) : zero4;
  float sx = p0.x, sy = p0.y, sz = p0.z;
  for (int base = 64; base < np; base += 64) {
    const float4 p = base + lane < np ? load(base + lane) : zero4;
    sx += p.x; sy += p.y; sz += p.z;
  }
  const float fn = (float)np;
  const float mx = __fdiv_rn(wave_sum_f(sx), fn), my = __fdiv_rn(wave_sum_f(sy), fn), mz = __fdiv_rn(wave_sum_f(sz), fn);
  // the centre columns of this fork: per-pillar constants (pillar_encoder.py:126-133)
  const float fcx = -((float)x * vx + xo);
  const float fcy = -((float)y * vy + yo);
  const float cbase = fmaf(w[8], fcy, w[7] * fcx);
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
      if (DIST) a = fmaf(w[K - 1], __fsqrt_rn(px * px + py * py + pz * pz), a);
      m = fmaxf(m, a * sc + sh);
    }
  }
  return m;
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
