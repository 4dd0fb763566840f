// One training batch's clouds and ground truth drawn from resident scene tables (sessd_draw_batch): the device form of the
// loader's per-frame torch arithmetic (sessd_hip/trainloop.py: DeviceBatcher._student_cloud, _student_boxes, _in_range), which is
// the global augmentation of det3d/datasets/pipelines/preprocess.py:137-140 (random flip about the x axis, rotation about z,
// scaling) followed by Voxelization's ground-truth range filter (core/sampler/preprocess.py:138-148).
// Two launches per batch, whatever its size:
//   points  grid (ceil(P / 256), B), one 16-byte row per thread: rows below the scene's count are moved, the rest become the
//           out-of-range row sessd_stage_points pads with. No LDS.
//   boxes   one 128-thread block per frame (G <= 128): every live box is moved, kept when any of its four BEV corners lies
//           strictly inside the range, and the kept rows are compacted in row order (ballot prefix over the block's two
//           waves); classes travel with their rows; rows at or beyond the kept count are zeros; the frame's [flipped, cos,
//           sin, rotation, scale] row is copied out; the count is written last.
// Every product and sum is rounded once, in the order the torch formulation has them (__fmul_rn / __fadd_rn: nothing here
// may contract to an FMA, whatever the file is compiled with). cosf / sinf of the moved yaw feed the keep decision only.
// Which row of the (T, B) tables is used comes from a host integer or from a device counter, modulo T, so a replayed launch
// can never index outside the tables; a scene index outside [0, S) draws an empty frame.
#include "common.hpp"

namespace {

constexpr int PT_NT = 256;
constexpr int BOX_NT = 128;
constexpr float PI_F = 3.14159274101257324f;  // float32(pi)

struct DrawTables {
  const float4* pool_points;   // (S, P)
  const int* pool_point_count; // (S)
  const float* pool_boxes;     // (S, G, 7)
  const int* pool_classes;     // (S, G)
  const int* pool_box_count;   // (S)
  const int* choice;           // (T, B)
  const float* par;            // (T, B, 5)
  const int* iter_dev;         // device counter or null
  int S, P, G, T, B, iter_host;
  float lo_x, lo_y, hi_x, hi_y;
};

__device__ __forceinline__ int table_row(const DrawTables& D) {
  const int it = D.iter_dev ? *D.iter_dev : D.iter_host;
  const int r = it % D.T;
  return r < 0 ? r + D.T : r;
}

struct Move {
  bool flip;
  float c, s, rot, k;
};

__device__ __forceinline__ Move load_move(const DrawTables& D, int row, int b) {
  const float* p = D.par + ((size_t)row * D.B + b) * 5;
  Move m;
  m.flip = p[0] != 0.f;
  m.c = p[1]; m.s = p[2]; m.rot = p[3]; m.k = p[4];
  return m;
}

// DeviceBatcher._move: flip about the x axis, rotate, scale
__device__ __forceinline__ void move_xy(const Move& m, float x, float y, float* X, float* Y) {
  const float yf = m.flip ? -y : y;
  *X = __fmul_rn(__fadd_rn(__fmul_rn(x, m.c), __fmul_rn(yf, m.s)), m.k);
  *Y = __fmul_rn(__fadd_rn(__fmul_rn(-x, m.s), __fmul_rn(yf, m.c)), m.k);
}

__global__ __launch_bounds__(PT_NT) void draw_points_kernel(DrawTables D, float4* __restrict__ staged) {
  const int b = blockIdx.y, i = blockIdx.x * PT_NT + threadIdx.x;
  if (i >= D.P) return;
  const int row = table_row(D);
  const int scene = D.choice[(size_t)row * D.B + b];
  const bool ok = scene >= 0 && scene < D.S;
  const int n = ok ? min(max(D.pool_point_count[scene], 0), D.P) : 0;
  float4 v = make_float4(-1.0e6f, -1.0e6f, -1.0e6f, 0.f);
  if (i < n) {
    const Move m = load_move(D, row, b);
    const float4 p = D.pool_points[(size_t)scene * D.P + i];
    move_xy(m, p.x, p.y, &v.x, &v.y);
    v.z = __fmul_rn(p.z, m.k);
    v.w = p.w;
  }
  staged[(size_t)b * D.P + i] = v;
}

// DeviceBatcher._in_range on one moved box: any corner strictly inside the range
__device__ __forceinline__ bool any_corner_inside(const DrawTables& D, const float* v) {
  const float c = cosf(v[6]), s = sinf(v[6]);
  const float fx[4] = {-0.5f, -0.5f, 0.5f, 0.5f}, fy[4] = {-0.5f, 0.5f, 0.5f, -0.5f};
  bool keep = false;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float dx = __fmul_rn(fx[q], v[3]), dy = __fmul_rn(fy[q], v[4]);
    const float x = __fadd_rn(__fadd_rn(__fmul_rn(dx, c), __fmul_rn(dy, s)), v[0]);
    const float y = __fadd_rn(__fadd_rn(__fmul_rn(-dx, s), __fmul_rn(dy, c)), v[1]);
    keep = keep || (x > D.lo_x && x < D.hi_x && y > D.lo_y && y < D.hi_y);
  }
  return keep;
}

__global__ __launch_bounds__(BOX_NT) void draw_boxes_kernel(DrawTables D, float* __restrict__ gt_boxes, int* __restrict__ gt_classes,
                                                             int* __restrict__ gt_count, float* __restrict__ transformation) {
  __shared__ int scnt[2];
  const int b = blockIdx.x, tid = threadIdx.x, G = D.G;
  const int row = table_row(D);
  const int scene = D.choice[(size_t)row * D.B + b];
  const bool ok = scene >= 0 && scene < D.S;
  const int n = ok ? min(max(D.pool_box_count[scene], 0), G) : 0;
  if (tid < 5) transformation[b * 5 + tid] = D.par[((size_t)row * D.B + b) * 5 + tid];
  float v[7];
  int cls = 0;
  bool keep = false;
  if (tid < n) {
    const Move m = load_move(D, row, b);
    const float* g = D.pool_boxes + ((size_t)scene * G + tid) * 7;
    move_xy(m, g[0], g[1], &v[0], &v[1]);
#pragma unroll
    for (int q = 2; q < 6; ++q) v[q] = __fmul_rn(g[q], m.k);
    const float yaw = m.flip ? __fadd_rn(-g[6], PI_F) : g[6];
    v[6] = __fadd_rn(yaw, m.rot);
    cls = D.pool_classes[(size_t)scene * G + tid];
    keep = any_corner_inside(D, v);
  }
  // kept rows in row order: ballot prefix over the two waves (as assign_target.hip compacts its class filter)
  const unsigned long long mask = __ballot(keep);
  if ((tid & 63) == 0) scnt[tid >> 6] = __popcll(mask);
  __syncthreads();
  const int kept = scnt[0] + scnt[1];
  float* ob = gt_boxes + (size_t)b * G * 7;
  int* oc = gt_classes + (size_t)b * G;
  if (keep) {  // row k <= tid, written by this thread alone
    const int k = (tid >= 64 ? scnt[0] : 0) + __popcll(mask & ((1ull << (tid & 63)) - 1ull));
#pragma unroll
    for (int q = 0; q < 7; ++q) ob[k * 7 + q] = v[q];
    oc[k] = cls;
  }
  if (tid >= kept && tid < G) {  // rows no kept box lands in
#pragma unroll
    for (int q = 0; q < 7; ++q) ob[tid * 7 + q] = 0.f;
    oc[tid] = 0;
  }
  __syncthreads();
  if (tid == 0) gt_count[b] = kept;
}

}  // namespace

extern "C" {

int sessd_draw_batch(const float* pool_points, const int32_t* pool_point_count, const float* pool_boxes, const int32_t* pool_classes,
                     const int32_t* pool_box_count, const int32_t* choice, const float* par, int num_scenes, int points_per_scene,
                     int boxes_per_scene, int num_iterations, int batch, const float* range_xy, int iter_host, const int32_t* iter_dev,
                     float* staged, float* gt_boxes, int32_t* gt_classes, int32_t* gt_count, float* transformation,
                     hipStream_t stream) {
  if (num_scenes < 1 || points_per_scene < 1 || boxes_per_scene < 1 || boxes_per_scene > BOX_NT || num_iterations < 1 || batch < 1 ||
      batch > 65535)
    return SESSD_EINVAL;
  if ((long long)num_scenes * points_per_scene >= (1ll << 29) || (long long)batch * points_per_scene >= (1ll << 29) ||
      (long long)num_iterations * batch >= (1ll << 28))
    return SESSD_EINVAL;
  if (!pool_points || !pool_point_count || !pool_boxes || !pool_classes || !pool_box_count || !choice || !par || !range_xy || !staged ||
      !gt_boxes || !gt_classes || !gt_count || !transformation)
    return SESSD_EINVAL;
  if ((((size_t)pool_points | (size_t)staged) & 15) != 0) return SESSD_EINVAL;
  DrawTables D;
  D.pool_points = (const float4*)pool_points; D.pool_point_count = pool_point_count;
  D.pool_boxes = pool_boxes; D.pool_classes = pool_classes; D.pool_box_count = pool_box_count;
  D.choice = choice; D.par = par; D.iter_dev = iter_dev;
  D.S = num_scenes; D.P = points_per_scene; D.G = boxes_per_scene; D.T = num_iterations; D.B = batch; D.iter_host = iter_host;
  D.lo_x = range_xy[0]; D.lo_y = range_xy[1]; D.hi_x = range_xy[2]; D.hi_y = range_xy[3];
  SESSD_LAUNCH(draw_points_kernel, dim3(sessd_divup(D.P, PT_NT), D.B), dim3(PT_NT), 0, stream, D, (float4*)staged);
  SESSD_CHECK_LAUNCH();
  SESSD_LAUNCH(draw_boxes_kernel, dim3(D.B), dim3(BOX_NT), 0, stream, D, gt_boxes, gt_classes, gt_count, transformation);
  SESSD_CHECK_LAUNCH();
  return SESSD_OK;
}

}  // extern "C"
