/* Any input size: rectangular images and resampled position embeddings.  Additive to rajni_hip.h: no record, enum, entry
 * point or workspace size of that header (or of rajni_hip_layers.h) changes, and RAJNI_ABI_VERSION stays what it is.
 *
 * Images are [B, Cin, H, W] with H and W multiples of the patch size; the token grid is gh x gw = (H / patch) x (W / patch),
 * row-major (patch (y, x) is token y * gw + x behind the prefix tokens).  Nothing behind the embedding depends on the grid's
 * shape, only on the token count. */
#ifndef RAJNI_HIP_IMAGE_H
#define RAJNI_HIP_IMAGE_H

#include "rajni_hip_layers.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RAJNI_RESAMPLE_MAX_GRID 128 /* grids of 1..128 per axis on both sides: 16384 patch rows, the forward's token cap */

typedef struct {
  int height, width; /* pixels */
} rajni_vit_image;

/* Position-embedding resample, timm's resample_abs_pos_embed: src [prefix_rows + src_h * src_w, C] -> dst
 * [prefix_rows + dst_h * dst_w, C], both in `dtype` (bf16, fp16 or fp32), 16-byte aligned, C % 8 == 0.  The prefix rows are
 * copied bit for bit.  Patch rows: source -> fp32 -> bicubic (Keys, a = -0.5) with antialiasing, separable, as
 * F.interpolate(mode="bicubic", antialias=True, align_corners=False) computes it -> ONE rounding to `dtype`.  Per axis with
 * scale = n_in / n_out: support = 2 * max(scale, 1), centre c = scale * (i + 0.5), taps j in
 * [max(0, int(c - support + 0.5)), min(int(c + support + 0.5), n_in)) with weights k((j - c + 0.5) / max(scale, 1)) divided by
 * their sum.  The weight tables are evaluated in fp64 and rounded once to fp32; accumulation is fp32 FMA, source rows outer,
 * source columns inner, ascending.  Equal grids give the source's bits.  One launch, no atomics, no memset, every output
 * byte written exactly once, bit-repeatable.
 * Refused (RAJNI_ERR_UNSUPPORTED): a grid axis outside 1..RAJNI_RESAMPLE_MAX_GRID on either side - the message states the
 * cap - and C % 8 != 0; (RAJNI_ERR_INVALID): null or misaligned pointers, prefix_rows outside 0..RAJNI_MAX_PREFIX, a bad
 * dtype. */
int rajni_resample_pos_embed(const void* src, int src_h, int src_w, void* dst, int dst_h, int dst_w, int C, int prefix_rows,
                             int dtype, rajni_stream_t stream);

/* rajni_patch_embed_prefix for images [B, Cin, H, W]: x [B, num_prefix + (H / P) * (W / P), C]; `pos` holds
 * (num_prefix if pos_has_cls else 0) + (H / P) * (W / P) rows.  H == W == S is rajni_patch_embed_prefix launch for launch. */
int rajni_patch_embed_image(const void* images, const void* w, const float* bias, const void* cls, const void* reg,
                            int num_prefix, const void* pos, int pos_has_cls, void* x, int x_f32, int B, int Cin, int H, int W,
                            int P, int C, int dtype, void* workspace, size_t workspace_bytes, rajni_stream_t stream);
size_t rajni_patch_embed_workspace_bytes_image(int B, int Cin, int H, int W, int P, int dtype);

/* The forward of rajni_vit_forward_layers on images [B, in_chans, image.height, image.width].  image == NULL: exactly the
 * launches of that entry point and the same bits; image = {S, S} with plan.img_size == S likewise.  Otherwise the sequence
 * has n0 = (height / patch) * (width / patch) + P tokens and plan.pos_embed must hold the rows of that grid
 * (rajni_resample_pos_embed makes them); every count the other records speak of (keep, slabs, dense outputs) is against that
 * n0.  ext, prefix and layers may each be NULL.
 * Refused before the first launch and before the workspace check (RAJNI_ERR_INVALID): height or width <= 0 or not a multiple
 * of plan.patch_size, plan.img_size != height; (RAJNI_ERR_UNSUPPORTED): more than 16416 tokens. */
size_t rajni_vit_workspace_bytes_image(const rajni_vit_plan* plan, const rajni_vit_prefix* prefix, const rajni_vit_image* image);
int rajni_vit_forward_image(const rajni_vit_plan* plan, const rajni_vit_ext* ext, const rajni_vit_prefix* prefix,
                            const rajni_vit_layers* layers, const rajni_vit_image* image, const void* images, void* logits,
                            rajni_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* RAJNI_HIP_IMAGE_H */
