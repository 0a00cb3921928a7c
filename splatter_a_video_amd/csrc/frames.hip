// One call per direction for a whole frame batch (SURVEY 7 stage 6): the sequences FrameBatch (frames.py) composes from the
// *_batch entry points, for callers that want a single crossing of the C ABI per gradient step -- static Gaussians +
// per-frame offsets under the orthographic camera, one feature set.  Every buffer is caller-owned (splat_frames_t holds
// the pointers); nothing is allocated, nothing synchronises with the host.
#include "common.h"

static splat_camera_t batch_camera(const splat_frames_t *b) {
    splat_camera_t cam;
    memset(&cam, 0, sizeof(cam));
    cam.perspective = b->perspective; cam.intr = b->intr; cam.intr_frame_stride = b->intr_frame_stride;
    cam.extr = b->extr; cam.extr_frame_stride = b->extr_frame_stride; cam.offsets = b->offsets;
    return cam;
}

// pairs per tile and frame; with b->reach only the pairs whose tile the splat can reach (binning.hip: "reach masks")
static int frames_bin_count(const splat_frames_t *b) {
    if (b->reach) {
        SPLAT_CHECK_ARG(b->opacity != nullptr, "reach masks need the opacity");
        return splat_bin_count_batch_reach(b->F, b->P, b->uv, b->radius, b->conic, b->opacity, 0, b->W, b->H, b->bin_scratch,
                                           b->tile_range, b->pairs, nullptr, b->reach, b->stream);
    }
    return splat_bin_count_batch(b->F, b->P, b->uv, b->radius, b->W, b->H, b->bin_scratch, b->tile_range, b->pairs, b->stream);
}

extern "C" int splat_frames_forward(const splat_frames_t *b) {
    SPLAT_CHECK_ARG(b != nullptr && b->struct_bytes == sizeof(splat_frames_t), "splat_frames_t of another ABI version");
    SPLAT_CHECK_ARG(b->capacity >= 1, "capacity (pairs reserved per frame) must be set: run splat_frames_count first");
    const splat_camera_t cam = batch_camera(b);
    int rc = splat_preprocess_forward_batch_cam(b->F, b->P, b->xyz, b->offsets, b->scales, b->uquats, &cam, b->W, b->H,
                                                b->nearest, b->extent, b->uv, b->depth, b->conic, b->radius, b->stream);
    if (rc != SPLAT_OK) return rc;
    rc = frames_bin_count(b);
    if (rc != SPLAT_OK) return rc;
    if (b->reach)
        rc = splat_bin_sort_batch_reach(b->F, b->P, b->uv, b->depth, b->radius, b->reach, b->W, b->H, b->bin_scratch,
                                        b->tile_range, b->capacity, b->keys, b->idx_sorted, b->overflow, b->goff_incl, b->owner,
                                        b->slot_sorted, b->stream);
    else
        rc = splat_bin_sort_batch(b->F, b->P, b->uv, b->depth, b->radius, b->W, b->H, b->bin_scratch, b->tile_range, b->capacity,
                                  b->keys, b->idx_sorted, b->overflow, b->goff_incl, b->owner, b->slot_sorted, b->stream);
    if (rc != SPLAT_OK) return rc;
    return splat_alpha_blending_forward_batch(b->F, b->P, b->C, b->uv, b->conic, b->opacity, 0, b->feature, 0, b->idx_sorted,
                                              b->tile_range, b->capacity, b->bg, nullptr, b->W, b->H, 0, 0, b->out, b->final_T,
                                              b->ncontrib, nullptr, b->pack, b->cull_flags, b->stream);
}

// geometry + pair counts only: pairs[F] (device) tells the caller how much capacity to reserve before the first
// splat_frames_forward
extern "C" int splat_frames_count(const splat_frames_t *b) {
    SPLAT_CHECK_ARG(b != nullptr && b->struct_bytes == sizeof(splat_frames_t), "splat_frames_t of another ABI version");
    const splat_camera_t cam = batch_camera(b);
    int rc = splat_preprocess_forward_batch_cam(b->F, b->P, b->xyz, b->offsets, b->scales, b->uquats, &cam, b->W, b->H,
                                                b->nearest, b->extent, b->uv, b->depth, b->conic, b->radius, b->stream);
    if (rc != SPLAT_OK) return rc;
    return frames_bin_count(b);
}

// ------------------------------------------------------------------ wide detached sets beside the row
// After the tile backward of one 32-channel chunk of a wide set every pair owns a TAIL record [ux uy ca cb cc o | cn feature
// terms | pad] (NQ 16-byte chunks) at frame * cap + slot, a Gaussian's slots of one frame being contiguous and consecutive
// Gaussians' ranges adjacent (goff = inclusive prefix per frame).  NQ neighbouring lanes own one Gaussian, lane q the chunk q of
// every one of its records: a wave streams whole consecutive records with 16-byte loads.  Chunk 0 (ux uy ca cb) and float 4 (cc)
// go into the ROW's record at the same slot -- the slot has one owner, a plain read-modify-write; `o` is left out (detached
// opacity) -- and the chunks that hold feature terms are summed over the Gaussian's slots and the frames in ascending order and
// added to its d_feature row.  No float atomics.
struct WideFoldArgs {
    int F, P, cn, NQ;       // NQ = tail stride in 16-byte chunks
    long long cap;
    const int *goff;        // [F, P]
    const float4 *tail;     // [F, cap, NQ]
    float *row;             // [F, cap, RS]
    int RS;
    float *dfeat;           // NULL: geometry only
    long long dstride;
    int c0;
};

constexpr int WIDE_FOLD_U = 4;   // records a lane requests together (a Gaussian touches 2.6 tiles per frame on the bench scene)

__global__ void __launch_bounds__(256)
frames_wide_fold_kernel(const WideFoldArgs A) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(t / A.NQ), q = (int)(t - (long long)i * A.NQ);
    if (i >= A.P) return;
    const int f0 = blockIdx.y, fstep = gridDim.y;   // (the feature sum walks all frames: the host launches gridDim.y = 1 then)
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int f = f0; f < A.F; f += fstep) {
        const int *goff = A.goff + (size_t)f * A.P;
        long long b = i > 0 ? goff[i - 1] : 0, e = goff[i];
        if (e > A.cap) e = A.cap;   // a frame that outgrew the capacity dropped its surplus pairs
        if (b < 0) b = 0;
        const float4 *tail = A.tail + (size_t)f * (size_t)A.cap * A.NQ + q;
        float *row = A.row + (size_t)f * (size_t)A.cap * A.RS;
        for (long long s = b; s < e; s += WIDE_FOLD_U) {
            float4 v[WIDE_FOLD_U];
#pragma unroll
            for (int u = 0; u < WIDE_FOLD_U; ++u)
                v[u] = s + u < e ? tail[(size_t)(s + u) * A.NQ] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int u = 0; u < WIDE_FOLD_U; ++u) {
                if (s + u >= e) break;
                if (q == 0) {          // ux uy ca cb: one 16-byte read-modify-write of the row's record
                    float4 *r = reinterpret_cast<float4 *>(row + (size_t)(s + u) * A.RS);
                    float4 x = *r;
                    x.x += v[u].x; x.y += v[u].y; x.z += v[u].z; x.w += v[u].w;
                    *r = x;
                } else {
                    if (q == 1) row[(size_t)(s + u) * A.RS + REC_CC] += v[u].x;   // cc; `o` (float 5) stays out
                    acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w;
                }
            }
        }
    }
    if (!A.dfeat || q == 0) return;
    float *d = A.dfeat + (size_t)i * A.dstride + A.c0;
    const float a4[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = 4 * q + j - REC_GEOM;   // channel of the chunk held at float 4 q + j of the record
        if (k >= 0 && k < A.cn) d[k] += a4[j];
    }
}

extern "C" int splat_frames_wide_fold(int F, int P, int cn, int64_t capacity, const int32_t *goff_incl, const float *tail_records,
                                      float *row_records, int row_stride, float *d_feature, int64_t d_feature_stride, int c0,
                                      splat_stream_t stream) {
    SPLAT_CHECK_ARG(F >= 1 && P >= 1 && cn >= 1 && cn <= 32 && capacity >= 1 && c0 >= 0, "bad sizes (1 <= cn <= 32)");
    SPLAT_CHECK_ARG(row_stride >= 8 && (row_stride & 3) == 0, "bad sizes (row_stride: a multiple of 4 floats, >= 8)");
    SPLAT_CHECK_ARG(!d_feature || d_feature_stride >= (int64_t)c0 + cn, "bad sizes (d_feature_stride < c0 + cn)");
    SPLAT_CHECK_ARG(goff_incl && tail_records && row_records, "null pointer");
    SPLAT_CHECK_ARG((((uintptr_t)tail_records | (uintptr_t)row_records) & 15) == 0, "records must be 16-byte aligned");
    WideFoldArgs A;
    memset(&A, 0, sizeof(A));
    A.F = F; A.P = P; A.cn = cn; A.cap = capacity;
    A.NQ = (int)splat_blend_pair_stride(cn, 0, 0) / 4;
    A.goff = goff_incl; A.tail = (const float4 *)tail_records; A.row = row_records; A.RS = row_stride;
    A.dfeat = d_feature; A.dstride = d_feature_stride; A.c0 = c0;
    const long long threads = (long long)P * A.NQ;
    SPLAT_CHECK_ARG((threads + 255) / 256 < (1ll << 31), "bad sizes (too many Gaussians)");
    // the feature sum needs ONE owner per Gaussian over all frames (fixed order, no atomics): the frames are walked inside the
    // kernel; without a feature gradient the frame is a grid dimension
    const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)(d_feature ? 1 : (F < 65535 ? F : 65535)));
    SPLAT_LAUNCH("wide_fold", frames_wide_fold_kernel, grid, dim3(256), 0, (hipStream_t)stream, A);
    SPLAT_POST_LAUNCH();
    return SPLAT_OK;
}

extern "C" int splat_frames_backward(const splat_frames_t *b) {
    SPLAT_CHECK_ARG(b != nullptr && b->struct_bytes == sizeof(splat_frames_t), "splat_frames_t of another ABI version");
    SPLAT_CHECK_ARG(b->dL_dout && b->pair_records, "null pointer");
    // everything the second launch sequence validates is checked BEFORE the tile kernels run: a bad struct must not leave
    // half a backward behind (pair records overwritten, no gradients)
    SPLAT_CHECK_ARG(b->d_opacity && b->d_feature, "null gradient pointer");
    SPLAT_CHECK_ARG(b->d_xyz && b->d_scales && b->d_uquats, "null gradient pointer");
    SPLAT_CHECK_ARG(b->xyz && b->scales && b->uquats && b->extr && b->goff_incl && b->radius, "null pointer");
    SPLAT_CHECK_ARG(!b->perspective || b->intr, "the pinhole camera needs intr");
    SPLAT_CHECK_ARG(b->F == 1 || b->offsets || b->extr_frame_stride != 0, "several frames need per-frame offsets or cameras");
    int rc = splat_alpha_blending_backward_batch(b->F, b->P, b->C, b->idx_sorted, b->tile_range, b->capacity, b->bg, b->W, b->H,
                                                 b->final_T, b->ncontrib, b->dL_dout, b->want_abs, b->slot_sorted,
                                                 b->pair_records, b->pack, b->cull_flags, b->dbg_T_front, b->stream);
    if (rc != SPLAT_OK) return rc;
    const splat_camera_t cam = batch_camera(b);
    return splat_frames_gauss_backward_static_cam(b->F, b->P, b->C, b->W, b->H, b->capacity, b->want_abs, b->pair_records,
                                                  b->goff_incl, b->radius, b->xyz, b->scales, b->uquats, &cam, b->accumulate,
                                                  b->d_xyz, b->d_scales, b->d_uquats, b->d_opacity, b->d_feature, b->C, 0, -1,
                                                  b->tap, b->abs_tap, b->radii_max, b->stream);
}
