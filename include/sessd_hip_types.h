/* Plain-C argument structs of libsessd_hip.so (included by sessd_hip.h and by the kernels' sources). */
#ifndef SESSD_HIP_TYPES_H
#define SESSD_HIP_TYPES_H

#include <stddef.h>
#include <stdint.h>

/* One strided SparseConv3d step of a chain of sparse levels: level l-1 -> level l (level 0 = the voxels). */
typedef struct {
  int32_t ksize[3], stride[3], pad[3]; /* (z, y, x); ksize >= stride */
  int32_t out_dims[3];                 /* spatial shape (D, H, W) of level l */
  int32_t cap;                         /* row capacity of level l */
  int32_t* indices;                    /* out: (cap, 4) int32 [b, z, y, x], rows in ascending (b, z, y, x) order */
  int32_t* n_dev;                      /* out: live rows of level l (device int) */
} sessd_chain_level_t;

/* One neighbour table ("rulebook") over the output sites of `out_level`, looked up among the sites of `in_level`
 * (submanifold conv: in_level == out_level, stride 1, pad = ksize / 2). */
typedef struct {
  int32_t in_level, out_level;
  int32_t ksize[3], stride[3], pad[3];
  int32_t* nbr;        /* out: (kernel_volume, cap of out_level) input row or -1 */
  uint32_t* tile_mask; /* out: ceil(cap / 16) words, bit k = some site of the 16-site tile has a neighbour at offset k */
  /* optional (all three or none): OFFSET-PATTERN TILES. site_mask: out, (cap) words, bit k = site has a neighbour at offset k.
   * perm: out, ceil(cap / 256) * 256 bytes -- inside every group of 256 consecutive rows the live sites sorted by site_mask;
   * position p of the group holds row  group * 256 + perm[group * 256 + p]. tile_mask_sorted: out, ceil(cap / 256) * 16 words,
   * the tile masks of the 16-position tiles of that order. sessd_sparse_conv_sorted walks these tiles: sites with the same
   * neighbour pattern share a tile, so fewer (tile, offset) steps multiply rows without a neighbour -- same results per site. */
  uint32_t* site_mask;
  uint8_t* perm;
  uint32_t* tile_mask_sorted;
} sessd_rulebook_job_t;

/* One weight packing of a batched re-pack launch (sessd_dense_pack_batch): the arguments of sessd_conv2d_pack_taps (kind 0) or
 * sessd_conv3x3_winograd_pack (kind 1) plus the first block of the job inside the launch (256 threads per block; a job takes
 * ceil(elements / 256) blocks, elements = (cin/2) * ntaps * 2 * cout_pad32 for kind 0, cout_pad * cin for kind 1). */
typedef struct {
  const float* w;
  float* out;
  long long out_stride, in_stride;
  int32_t tap_off[16];
  int32_t cout, cin, ntaps;
  int32_t kind, flip, layout;
  int32_t block_start, pad_;
} sessd_dense_pack_job_t;

/* The three argument groups every dense launch entry shares (sessd_hip.h, "dense BEV neck"). An entry takes them as HOST
 * pointers and reads them before it returns; the pointers inside are DEVICE pointers. */
typedef struct {
  const float* scale;     /* device [cout] or NULL (1): the folded BatchNorm, out = act(conv * scale + shift) + residual */
  const float* shift;     /* device [cout] or NULL (0) */
  const float* residual;  /* device, the shape of the output, or NULL: added after the activation */
  int32_t relu;           /* != 0: act = max(., 0) */
} sessd_conv_epilogue_t;

/* The 2x2 tiles a list launch computes (sessd_bev_tile_activity builds both arrays): tiles[0 .. min(*count, cap)), entries
 * image * tiles per image + tile. A NULL sessd_tile_list_t* means the whole map; one without tiles, count or with cap < 1 is
 * refused. */
typedef struct {
  const int32_t* tiles;   /* device [cap] */
  const int32_t* count;   /* device, one int */
  int32_t cap;
} sessd_tile_list_t;

/* The stream-K block of sessd_conv3x3_winograd_sk / sessd_conv2d_sk. */
typedef struct {
  void* workspace;        /* device, the entry's *_workspace_bytes(), zeroed ONCE by the caller */
  size_t workspace_bytes;
  int32_t workgroups;     /* persistent workgroups: a multiple of 8, 0 = the kernel's default */
  int32_t min_rounds;     /* read only with a tile list: a share of the round list holds at least this many rounds (< 1: 1);
                             sessd_conv3x3_winograd_sk also takes -k: whole-unit shares of at least k units */
} sessd_stream_k_t;

/* One layer of sessd_fill_inactive_tiles: out (batch, cout, h, w), value[cout], tile_mask[batch][mask_th][2] 64-bit words (bit tx of
 * a row's 128 bits set = computed tile; mask_th >= h/2 rows per image), as sessd_bev_tile_activity writes them. */
typedef struct {
  float* out;
  const float* value;
  const uint64_t* tile_mask;
  int32_t cout, h, w, mask_th;
  int32_t tile;   /* 0 / 2: 2x2-pixel tiles, value[cout]; 4: 4x4-pixel tiles (a transposed conv over 2x2 tiles of its input),
                     value[4][cout] = the constant of each output parity class (py * 2 + px); 6: 2x2-pixel tiles with such a
                     value[4][cout] table (a 3x3 layer behind the transposed convs: its input is constant per parity class) */
  int32_t near_kind;           /* how near_mask's reader reaches this map: 0 = a 3x3 stride-1 layer on the SAME tile grid (reach:
                                  the 3x3 tiles around a listed tile); on a grid TWICE AS COARSE: 1 = it touches the map inside its
                                  listed tiles only (a residual), 2 = a 3x3 stride-2 layer over 2x2 tiles of its output (reach:
                                  tiles 2Ty-1 .. 2Ty+1, 2Tx-1 .. 2Tx+1 of this map) */
  const uint64_t* near_mask;   /* NULL, or (tile 2 only) the tile mask of the list-driven reader(s) of `out`: only the tiles within
                                  its reach are filled, the others keep what they hold */
} sessd_fill_tiles_job_t;

/* One sparse-conv weight packing of sessd_sparse_pack_batch: sessd_sparse_pack_weight (adjoint 0) or
 * sessd_sparse_pack_weight_adjoint (adjoint 1; reverse_k = its reverse_offsets); cin / cout are those of the STORED weight
 * (kernel_volume, cin, cout); a job takes ceil(kernel_volume * cin * cout / 256) blocks. */
typedef struct {
  const float* w;
  float* out;
  int32_t kernel_volume, cin, cout, adjoint, reverse_k, block_start;
} sessd_sparse_pack_job_t;

/* The head outputs and targets of ONE network (student or EMA teacher) as sessd_head_loss reads them: A anchors per sample in
 * the reference's order (anchor = (y * W + x) * 2 + rotation), B samples. box / dir / iou / cls are the NHWC tensors that
 * MultiGroupHead.forward returns (mg_head_sessd.py:217-230), viewed as (B, A, 7) / (B, A, 2) / (B, A) / (B, A). */
typedef struct {
  const float* box;          /* (B, A, 7) box codes */
  const float* cls;          /* (B, A) class logits (one class) */
  const float* dir;          /* (B, A, 2) direction logits */
  const float* iou;          /* (B, A) IoU predictions */
  const void* labels;        /* (B, A) int32 or int64 (cfg.labels_i64): -1 ignore, 0 negative, > 0 positive */
  const float* reg_targets;  /* (B, A, 7) encoded regression targets */
  const float* anchors;      /* (B, A, 7) [x, y, z, w, l, h, r] */
} sessd_head_loss_net_t;

/* Shapes, capacities and the constants of examples/second/configs/config.py that sessd_head_loss needs. */
typedef struct {
  int32_t batch, num_anchors, labels_i64;
  int32_t pos_capacity;      /* positive anchors of the whole batch kept per network (more: flagged in record[48], dropped) */
  int32_t cons_capacity;     /* consistency candidates kept per sample and network (score >= score_thresh inside center_range) */
  float pos_cls_weight, neg_cls_weight;             /* loss_norm (NormByNumPositives) */
  float focal_alpha, focal_gamma, smooth_l1_sigma;  /* loss_cls, loss_bbox.sigma */
  float cls_loss_weight, loc_loss_weight, dir_loss_weight, direction_offset;
  float score_thresh, match_iou_thresh;             /* 0.3 (mg_head_sessd.py:653) and 0.7 (:573) */
  float center_range[6];                            /* post_center_range (mg_head_sessd.py:484) */
} sessd_head_loss_cfg_t;

/* ONE task of sessd_supervised_loss: the task's head outputs viewed as (B, A, 7) / (B, A) / (B, A, 2), its targets, and the
 * gradient buffers of the same shapes, which the call WRITES in every element. All device pointers; dir / grad_dir 8-byte
 * aligned. */
typedef struct {
  const float* box;          /* (B, A, 7) box codes */
  const float* cls;          /* (B, A) class logits (one class per task) */
  const float* dir;          /* (B, A, 2) direction logits */
  const void* labels;        /* (B, A) int32 or int64 (cfg.labels_i64): -1 ignore, 0 negative, 1 positive */
  const float* reg_targets;  /* (B, A, 7) encoded regression targets */
  const float* anchors;      /* (B, A, 7) [x, y, z, w, l, h, r]; only the yaw is read */
  float* grad_box;
  float* grad_cls;
  float* grad_dir;
} sessd_supervised_task_t;

/* Shapes and the constants of a SECOND / PointPillars config that sessd_supervised_loss needs. */
typedef struct {
  int32_t batch, num_anchors, num_tasks /* 1..4 */, labels_i64;
  float pos_cls_weight, neg_cls_weight;             /* loss_norm (NormByNumPositives) */
  float focal_alpha, focal_gamma, smooth_l1_sigma;  /* loss_cls, loss_bbox.sigma */
  float cls_loss_weight, loc_loss_weight, dir_loss_weight, direction_offset;
} sessd_supervised_loss_cfg_t;

/* Shapes of sessd_assign_targets_batch: B frames, A anchors per task, T tasks (1..4), G ground-truth rows per frame (1..128). */
typedef struct {
  int32_t batch, num_anchors, num_tasks, gt_capacity;
  int32_t labels_i64;        /* labels are int64 (else int32) */
  int32_t anchors_per_frame; /* 0: every task's anchors are (A, 7), shared by the frames; else (B, A, 7) */
} sessd_assign_batch_cfg_t;

/* ONE task of sessd_assign_targets_batch: its anchors, its class, its thresholds and the tensors the call WRITES in every
 * element. All device pointers. */
typedef struct {
  const float* anchors;      /* (A, 7), or (B, A, 7) when cfg.anchors_per_frame */
  int32_t class_id;          /* rows with gt_classes == class_id are this task's; <= 0: every live row (enable_similar_type) */
  float matched, unmatched;  /* positive at IoU >= matched, background below unmatched */
  void* labels;              /* (B, A) int32 or int64 per cfg.labels_i64: -1 ignore, 0 background, 1 positive */
  float* reg_targets;        /* (B, A, 7) */
  float* reg_weights;        /* (B, A) or NULL */
  int32_t* gt_id;            /* (B, A) or NULL: index among the task's rows of that frame in row order, -1 elsewhere */
} sessd_assign_task_t;

/* DI-NMS settings of sessd_predict (args->di): the arguments get_task_detections passes to box_torch_ops.rotate_weighted_nms
 * (mg_head_sessd.py:1012-1017: centerness_pow 2, nms_cnt_thresh 2.6, intervals (0, 20, 40, 60), sigma squares (0.0009, 0.009,
 * 0.1, 1), suppressed_thresh 0.3). interval[0 .. n_interval) are the distance bounds, sigma_sq[k] belongs to
 * [interval[k], interval[k + 1]): n_interval - 1 entries are read. */
typedef struct {
  float cnt_thresh, suppressed_thresh, centerness_pow;
  int32_t n_interval;        /* <= 8 */
  float interval[8], sigma_sq[8];
} sessd_di_cfg_t;

/* The arguments of sessd_predict (sessd_hip.h documents the launches and the DI-NMS semantics). B = batch, T = num_tasks,
 * A = 2 * num_pixels anchors per task, post = post_max_size. Every pointer is a device pointer except `di`; an optional one is
 * NULL when absent. */
typedef struct {
  /* inputs */
  const float* head;           /* (B, T, 22, num_pixels) planar float32: per task ch 0..13 box codes (7 per anchor), 14..15 cls,
                                  16..19 dir, 20..21 iou (one class and two rotations per task) */
  int32_t batch;
  int32_t num_tasks;           /* 1..4; (frame, task) runs as the virtual frame b * T + t */
  int32_t num_pixels;          /* H * W */
  const float* anchors;        /* (T, A, 7) shared by all frames, or (B, T, A, 7) */
  int32_t anchors_per_frame;   /* 0: shared anchors; A: per-frame anchors */
  const double* frustum;      /* (B, 1, 6, 4, 3) float64 per real frame, or NULL */
  /* settings: every task applies score_thresh, pre_max_size, the NMS and post_max_size on its own */
  float score_thresh;
  int32_t pre_max_size;        /* <= 1984; <= 1024 with di */
  int32_t post_max_size;
  float nms_iou_thresh;        /* with di: accepted and never read, like the reference's iou_threshold */
  float post_center_range[6];  /* by value */
  float direction_offset;
  /* outputs: rows [0, out_count[b]) are frame b's detections -- task 0's in NMS order, then task 1's, ...; label = task index */
  float* out_box;              /* (B, T * post, 7) */
  float* out_score;            /* (B, T * post) */
  int32_t* out_label;          /* (B, T * post) */
  int32_t* out_count;          /* (B,) */
  int32_t* out_task_count;     /* (B, T) or NULL: the rows each task contributed */
  /* optional, both or neither: the score-filter keys (B * T, A) uint64 and their per-(frame, task) counts already produced with
   * the head tensor (sessd_ssfa_fuse_head_tasks / sessd_rpn_up_head_tasks; anchor id local to the task) -- the count clear and
   * the score-filter launch are skipped */
  const uint64_t* ext_keys;
  const int32_t* ext_key_count;
  /* optional, all or none: every frame also leaves its fixed-size detection record (T * post, 9) from inside the call's last
   * launch, with the layout and ring rule of sessd_pack_detections: slot = (*cursor + b) % capacity_frames, *cursor += batch */
  float* records;              /* (capacity_frames, T * post, 9) */
  int32_t* record_counts;      /* (capacity_frames,) */
  int32_t capacity_frames;     /* >= batch; batch <= 256 */
  int32_t* cursor;             /* one device int */
  /* optional: DI-NMS instead of the greedy rotated NMS (NULL) */
  const sessd_di_cfg_t* di;    /* HOST pointer, read before the call returns */
  int32_t* di_truncated;       /* (B, T) or NULL: 1 where the selection stopped with unsuppressed candidates left, else 0 */
  int32_t* di_truncated_sticky;/* one int32 or NULL: 1 is ORed into it in that case, never cleared by the call */
  int32_t* di_keep;            /* (B * T, post) / di_keep_count (B * T), both or neither: the kept candidates' ranks in the */
  int32_t* di_keep_count;      /* frame's top-k order and their number, BEFORE the filters (the reference's `selected`) */
} sessd_predict_args_t;

#endif
