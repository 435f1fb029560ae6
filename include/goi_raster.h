/*
 * include/goi_raster.h -- C ABI of libgoi_raster.so, the MI355X (gfx950) differentiable Gaussian
 * rasterizer with a per-Gaussian semantic-feature channel.
 *
 * This is the drop-in boundary for the reference's rasterizer hot path.  Each entry point replaces
 * one C++ entry of the reference (paths relative to submodules/diff-gaussian-rasterization/):
 *
 *   goi_raster_forward      <- CudaRasterizer::Rasterizer::forward   cuda_rasterizer/rasterizer.h:20-46,
 *                              called from RasterizeGaussiansCUDA    rasterize_points.cu:35-123
 *   goi_raster_backward     <- CudaRasterizer::Rasterizer::backward  cuda_rasterizer/rasterizer.h:75-111,
 *                              called from RasterizeGaussiansBackwardCUDA rasterize_points.cu:213-306
 *   goi_raster_trace        <- CudaRasterizer::Rasterizer::trace     cuda_rasterizer/rasterizer.h:48-73,
 *                              called from TraceGaussiansCUDA        rasterize_points.cu:125-211
 *   goi_raster_mark_visible <- CudaRasterizer::Rasterizer::markVisible cuda_rasterizer/rasterizer.h:13-18,
 *                              called from markVisible               rasterize_points.cu:308-327
 *   goi_raster_*_bytes      <- required<GeometryState/ImageState/BinningState>() cuda_rasterizer/rasterizer_impl.h:67-73
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch tensors in the Python binding);
 *     no torch types cross this boundary; inputs are never written;
 *   - an absent optional input is NULL (the reference's "empty tensor => nullptr", rasterize_points.cu:98-111);
 *   - all arrays are contiguous fp32 unless stated; matrices are 16 floats in the reference's
 *     transposed (row-vector) convention (cuda_rasterizer/auxiliary.h:58-77);
 *   - the three workspaces are opaque bytes sized by goi_raster_*_bytes(); the binning workspace
 *     size depends on num_rendered, which is only known mid-call, so the caller passes an
 *     allocation callback (the reference's std::function<char*(size_t)>, rasterize_points.cu:27-33);
 *   - outputs need not be initialised by the caller; every element is written;
 *   - `stream` is a hipStream_t (NULL = the default stream); all work is enqueued on it; the only
 *     host synchronisation is the read-back of num_rendered inside forward/trace (the reference
 *     has the same one, cuda_rasterizer/rasterizer_impl.cu:285); goi_raster_forward_async has none;
 *   - entry points may be called concurrently from several host threads on different streams / devices
 *     (read-back tickets are pooled per device under a mutex; last_error is per thread); the
 *     goi_raster_set_option switches are process-wide but every call works with the snapshot it took when it
 *     started (a switch flipped by another thread never changes a call half-way); the stage profile is process-wide;
 *   - return value: >= 0 on success (forward/trace: num_rendered), < 0 on error with the message
 *     available from goi_raster_last_error() (thread-local).
 *   - supported S (semantic channels): any 1..32; fast paths are instantiated for 10 and 16.
 *   - alignment: device pointers as torch / hipMalloc hand them out (256 bytes) are always fine.  What the kernels actually
 *     assume: `semantics` 16-byte aligned when S is a multiple of 4 (its rows are moved as 16-byte words, by LDS-DMA in the
 *     backward), the workspaces 256-byte aligned, everything else 4 bytes.
 */
#ifndef GOI_RASTER_H
#define GOI_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 9: ONE ENTRY PER OPERATION of the rasterizer's frame (signatures change: nothing is added).  goi_raster_forward,
 *    goi_raster_forward_async, goi_raster_ticket_result and goi_raster_backward take the widest parameter list there was, and the
 *    seven names that carried the history are REMOVED: goi_raster_forward_selected, goi_raster_forward_async_selected,
 *    goi_raster_forward_async_cut, goi_raster_ticket_result2, goi_raster_backward2, goi_raster_backward3, goi_raster_backward4;
 *    goi_raster_forward_async refuses a selection together with a depth cut;
 *    later additions: goi_raster_contrib_votes; goi_knn_graph_workspace_bytes, goi_knn_graph, goi_knn_majority;
 *    goi_pose_gradient_workspace_bytes, goi_pose_gradient; goi_knn_transpose_workspace_bytes, goi_knn_transpose,
 *    goi_knn_smooth_loss_workspace_bytes, goi_knn_smooth_loss, goi_knn_diffuse; goi_knn_segment_edges,
 *    goi_knn_segment_components_workspace_bytes, goi_knn_segment_components; goi_instance_members_workspace_bytes,
 *    goi_instance_members, goi_instance_stats_workspace_bytes, goi_instance_stats; goi_mask_contrast_workspace_bytes,
 *    goi_mask_contrast; goi_mcmc_relocate_workspace_bytes, goi_mcmc_relocate, goi_mcmc_noise, goi_mcmc_debug_relocation_sum;
 *    goi_deform_solve_workspace_bytes, goi_deform_solve, goi_deform_energy_workspace_bytes, goi_deform_energy, goi_deform_apply
 * 8: + the two _selected forward entries (a per-Gaussian selection the forward itself honours; folded by 9);
 *    later additions: goi_semantic_pca_workspace_bytes, goi_semantic_pca_accumulate, goi_semantic_pca_solve,
 *    goi_semantic_pca_apply; goi_field_density_workspace_bytes, goi_field_density, goi_field_iso_workspace_bytes,
 *    goi_field_iso_count, goi_field_iso_emit; goi_mesh_components_workspace_bytes, goi_mesh_components,
 *    goi_mesh_clean_workspace_bytes, goi_mesh_clean_plan, goi_mesh_clean_emit, goi_mesh_decimate_workspace_bytes,
 *    goi_mesh_decimate_members, goi_mesh_decimate_probe, goi_mesh_decimate_plan, goi_mesh_decimate_emit,
 *    goi_mesh_normals_workspace_bytes, goi_mesh_normals; goi_texture_rasterize_workspace_bytes, goi_texture_rasterize,
 *    goi_texture_resolve, goi_texture_grid_put_workspace_bytes, goi_texture_grid_put, goi_texture_accumulate,
 *    goi_texture_normalize, goi_texture_fill_workspace_bytes, goi_texture_fill; goi_edit_bounds_workspace_bytes,
 *    goi_edit_bounds, goi_edit_transform; goi_raster_contrib_frame
 * 7: + the backward with prev_mask / row_mask (per-row mask of the rows a backward's chain wrote; folded by 9),
 *    goi_raster_debug_backward_contrib_offset, option bwd_skip_idle; the backward scratch grew by one byte per instance
 *    (contribution bytes: sizes come from goi_raster_backward_scratch_bytes as ever);
 *    later additions: goi_semantic_frame_workspace_bytes, goi_semantic_frame_compose
 * 6: + the backward with scratch_instances / flags (row scratch sized by the frame's count instead of its capacity; folded by 9),
 *    goi_raster_blend_stats;
 *    later additions: goi_semantic_osh_counts, goi_semantic_osh_fit, goi_semantic_dbscan_workspace_bytes, goi_semantic_dbscan,
 *    goi_semantic_mask_pack, goi_semantic_mask_dilate, goi_semantic_mask_unpack, goi_semantic_mask_confusion,
 *    goi_raster_debug_sort_workspace_bytes, goi_raster_debug_sort_pairs, goi_raster_debug_scan_workspace_bytes,
 *    goi_raster_debug_exclusive_scan; goi_knn_dist2 and goi_semantic_dbscan refuse 2^30 points or more;
 *    goi_raster_debug_reduce_row_floats, goi_raster_debug_reduce_workspace_bytes, goi_raster_debug_reduce_rows,
 *    goi_codebook_unique_rows_workspace_bytes, goi_codebook_unique_rows, goi_codebook_kmeans_workspace_bytes, goi_codebook_kmeans,
 *    goi_raster_photometric_workspace_bytes, goi_raster_photometric_forward, goi_raster_photometric_backward,
 *    goi_raster_debug_preprocess_backward, goi_raster_debug_pair_eval, goi_raster_debug_backward_blend
 * 5: + the _async forward with zcut_in / zcut_out and the ticket entry with the flag word (speculative depth cut-off of the tile
 *    lists), the backward with prev_radii (all three folded by 9); the binning and backward-scratch workspaces grew (member
 *    masks; descriptors of big Gaussians): sizes come from goi_raster_*_bytes as ever
 * 4: + goi_raster_truncated_flag, goi_adam_step_guarded; a truncated speculative frame back-propagates ZERO gradients
 * (3: + goi_raster_forward_reblend, goi_codebook_sim, goi_codebook_fused; 2: + the asynchronous forward; additions only) */
#define GOI_RASTER_ABI_VERSION 9

typedef struct GoiRasterScene {
    int P;                       /* number of Gaussians */
    int D;                       /* active SH degree, 0..3 */
    int M;                       /* SH coefficients per colour channel held in shs (0 if shs == NULL) */
    int S;                       /* semantic channels */
    int W, H;                    /* image width, height */
    const float* bg;             /* [3] */
    const float* means3D;        /* [P,3] */
    const float* shs;            /* [P,M,3] or NULL; 16-byte aligned when 3 M is a multiple of 4 (rows move as 16-byte words) */
    const float* colors_precomp; /* [P,3] or NULL */
    const float* semantics;      /* [P,S] (forward/backward) */
    const float* opacities;      /* [P] */
    const float* scales;         /* [P,3] or NULL */
    float scale_modifier;
    const float* rotations;      /* [P,4] (r,x,y,z) or NULL */
    const float* cov3D_precomp;  /* [P,6] or NULL */
    const float* viewmatrix;     /* [16] */
    const float* projmatrix;     /* [16] */
    const float* campos;         /* [3] */
    float tan_fovx, tan_fovy;
    int prefiltered;
    int debug;                   /* synchronise and check after every stage */
} GoiRasterScene;

/* Device-memory allocation callback: must return a device pointer to at least `bytes` bytes that
 * stays valid until the matching backward has run (NULL = failure). */
typedef void* (*goi_alloc_fn)(void* user, size_t bytes);

/* Thread safety: entry points may be called from several host threads (one per stream); the last-error
 * string and the pinned read-back buffer are per thread.  The profiling hooks and goi_raster_set_option touch
 * process-wide state and are meant for single-threaded measurement runs. */
int goi_raster_abi_version(void);
const char* goi_raster_last_error(void);

size_t goi_raster_geom_bytes(int P);
size_t goi_raster_image_bytes(int W, int H);
size_t goi_raster_binning_bytes(int num_rendered);
size_t goi_raster_backward_scratch_bytes(int num_rendered, int S);

/* Forward: color[3,H,W], semantic[S,H,W], depth[H,W], alpha[H,W], radii[P] (int32).  Returns num_rendered.
 *   geom_buffer, image_buffer : workspaces of goi_raster_geom_bytes(P) / goi_raster_image_bytes(W, H) bytes, uninitialised;
 *   binning_alloc, alloc_user : called once, with goi_raster_binning_bytes(num_rendered), when the host has read the count;
 *   keep, invert              : a SELECTION of the Gaussians, rendered in place (below); keep == NULL renders all of them.
 *
 * A SELECTION (the reference's viewer index-selects every per-Gaussian tensor by a boolean mask before it calls the rasterizer,
 * gui/gs_renderer.py:315-321: a host synchronisation, a second copy of the selected set, and outputs of the subset's length):
 *   keep   : [P] device bytes, one per Gaussian (never written; a torch.bool or torch.uint8 tensor as it is), or NULL;
 *   invert : 0 -- Gaussian i is rendered iff keep[i] != 0;  non-zero -- iff keep[i] == 0 (the complement, without forming it).
 * The frame is the frame of the selected Gaussians alone, bit for bit what a call with keep == NULL produces for the
 * index-selected arrays (outputs, num_rendered, and -- scattered to their ids -- radii and every gradient).  An unselected
 * Gaussian is dropped by the first kernel before anything of it but its selection byte is read, exactly where a Gaussian
 * behind the near plane is dropped: radii[i] = 0, no tile, no instance, zero gradient rows; it does not trip the
 * `prefiltered` check.  All arrays stay [P]-long and are indexed by the caller's own ids.
 * Everything that reads the geometry workspace -- goi_raster_forward_redo, _reblend, goi_raster_backward,
 * goi_raster_backward_semantics -- works behind a selected forward unchanged and takes no selection (a reblend shows the
 * selection of the frame that filled the workspaces).  goi_raster_forward_async takes the same pair; there is no selection
 * together with a depth cut, and no selected trace or mark_visible. */
int goi_raster_forward(const GoiRasterScene* scene, void* geom_buffer, void* image_buffer,
                       goi_alloc_fn binning_alloc, void* alloc_user,
                       float* out_color, float* out_semantic, float* out_depth, float* out_alpha,
                       int* radii, const uint8_t* keep, int invert, void* stream);

/* ---- Speculative forward: the same frame WITHOUT the host round trip -----------------------------------------------
 * (no counterpart in the reference: CudaRasterizer::Rasterizer::forward blocks on num_rendered at
 * cuda_rasterizer/rasterizer_impl.cu:285 to size the binning workspace; SURVEY.md section 7 "no host sync").
 *
 * goi_raster_forward_async enqueues the WHOLE frame and returns at once.  The caller supplies the binning workspace
 * up front, sized by goi_raster_binning_bytes(capacity) for a capacity it believes to be >= num_rendered (e.g. twice
 * the largest count seen so far); on the device every kernel takes the true count from the geometry workspace and
 * clamps it to `capacity`.  The return value is a TICKET (>= 0) for the asynchronous read-back of the count:
 *
 *   goi_raster_ticket_result(ticket, wait, &n, &flags): 1 = the count has arrived (n = num_rendered; the ticket is released),
 *       0 = not yet (only with wait == 0), -1 = error (e.g. the "prefiltered" trap; ticket released).
 *   n <= capacity : the frame is exactly what goi_raster_forward would have produced (bit-identical outputs; the
 *       tile lists are identical, only the workspace is larger).  Pass R = capacity to goi_raster_backward.
 *   n >  capacity : OVERFLOW.  The frame was rendered from the first `capacity` instances in emit (depth) order --
 *       memory-safe, but not the right image.  The device knows (emit sets the frame's "truncated" word in the
 *       geometry workspace, goi_raster_truncated_flag): goi_raster_backward / _backward_semantics on such a frame write
 *       ZERO into every gradient, so a truncated frame never trains anything even if the host has not looked at the
 *       count yet (the reference sizes its buffers from the true count and cannot truncate, CR/rasterizer_impl.cu:283-289);
 *       goi_adam_step_guarded can skip the optimiser step of that view on the device as well.
 *       goi_raster_forward_redo re-runs emit -> tile sort -> blend from the geometry state that is still in the
 *       workspace, into a binning buffer of goi_raster_binning_bytes(n) bytes: afterwards outputs and workspaces are
 *       bit-identical to goi_raster_forward's, and R = n.
 *
 * goi_raster_forward_redo reads only P, S, W, H, semantics and bg from `scene` (the other fields may be NULL).
 * Nothing here waits for the device unless asked to (wait != 0).  Every ticket must be resolved exactly once.
 * A resolved ticket means the COUNT has arrived -- it is final before the frame's blend kernel starts -- not that the frame's
 * kernels have finished: the outputs are ordered on `stream` like any other kernel's.  A blocking wait spins on host memory;
 * after two seconds it synchronises the frame's stream (not the device) and fails loudly rather than hang.
 * Not available with scene->debug (which synchronises after every stage) or for P == 0.
 *
 * keep, invert: the selection of goi_raster_forward (NULL, 0: every Gaussian).
 *
 * zcut_in, zcut_out: the SPECULATIVE DEPTH CUT-OFF of the tile lists (no counterpart in the reference, which lists every Gaussian
 * in every tile of its rectangle, CR/rasterizer_impl.cu:70-111, although a pixel stops at T < 1e-4, CR/forward.cu:352-357: on an
 * opaque scene three quarters of the instances lie behind their tile's saturation front and are emitted, sorted and never looked
 * at).  Two per-TILE arrays (ceil(W/16) * ceil(H/16) floats, row-major); both NULL is the frame without a cut:
 *   zcut_out (or NULL): LEARNT by this frame -- for every tile, the view depth up to which its list is worth listing the next
 *       time the same camera is rendered: the depth of the list entry a quarter (+ 64 positions) beyond the last position any
 *       pixel of the tile looked at; +inf for a tile in which some pixel reached the end of its list unsaturated.
 *   zcut_in (or NULL): APPLIED to this frame -- a Gaussian deeper than zcut_in[t] is not listed in tile t (rectangles of up to
 *       64 tiles, cull_variant 2: the cut lives in the ellipse tile masks).  Hand in what an earlier frame of the SAME camera
 *       learnt (never an uninitialised array).
 * A frame whose pixels all saturate inside their cut lists is bit-identical to the uncut frame: outputs, n_contrib, every
 * gradient (the dropped instances were never looked at).  If a pixel of a cut tile reaches the end of its list unsaturated, or
 * looks at an entry DEEPER than its tile's cut (a rectangle of more than 64 tiles has no tile mask and stays listed at every
 * depth: the Gaussians that were dropped in between would have come first), the cut was TOO TIGHT for this frame (the geometry
 * has moved since it was learnt): the forward blend raises bit 2 of the frame's flag word (goi_raster_truncated_flag; bit 0 = the
 * instance list was truncated, bit 1 = a sort timed out), the frame's backward writes ZERO gradients like a truncated frame's,
 * and goi_raster_ticket_result hands the word to the host, which renders the frame again without a cut (goi_raster_forward) and
 * forgets what the camera had learnt.
 * A selection and a cut do not go together: keep != NULL with zcut_in or zcut_out is refused.
 *
 * goi_raster_ticket_result: num_rendered (or NULL) receives the count, frame_flags (or NULL) the frame's flag word (GOI_FRAME_*;
 * 0 for a frame of goi_raster_forward); both are written only when the call returns 1. */
int goi_raster_forward_async(const GoiRasterScene* scene, void* geom_buffer, void* image_buffer, void* binning_buffer,
                             int capacity, float* out_color, float* out_semantic, float* out_depth, float* out_alpha,
                             int* radii, const float* zcut_in, float* zcut_out, const uint8_t* keep, int invert, void* stream);
int goi_raster_ticket_result(int ticket, int wait, int* num_rendered, unsigned* frame_flags);
#define GOI_FRAME_TRUNCATED 1u
#define GOI_FRAME_MISSORTED 2u
#define GOI_FRAME_CUT_TOO_TIGHT 4u
/* Device pointer (inside the geometry workspace of a frame over P Gaussians) of the frame's "truncated" word: non-zero
 * iff the frame's instance list did not fit its binning capacity.  Written by every forward (0 for goi_raster_forward
 * and after goi_raster_forward_redo); read on the device by the backward kernels and, if handed over, by
 * goi_adam_step_guarded.  NULL for P <= 0. */
const uint32_t* goi_raster_truncated_flag(const void* geom_buffer, int P);
int goi_raster_forward_redo(const GoiRasterScene* scene, int num_rendered, void* geom_buffer, void* image_buffer,
                            void* binning_buffer, float* out_color, float* out_semantic, float* out_depth,
                            float* out_alpha, const int* radii, void* stream);

/* The blend of a frame whose geometry and tile lists are already in workspaces filled by an earlier goi_raster_forward /
 * _async / _redo of the SAME camera over the SAME Gaussian geometry (positions, covariances, opacities, colours): only the
 * semantic rows and the background may have changed.  Runs the forward blend alone (no preprocess, sort or emit), writes the
 * four outputs and a fresh image workspace (`image_buffer`, goi_raster_image_bytes; the tile ranges are copied from
 * `cached_image_buffer`), and leaves geometry and binning workspaces untouched, so the result is what goi_raster_forward
 * would produce for the current semantics, bit for bit, and goi_raster_backward / _backward_semantics can follow with (geom, binning, the NEW
 * image workspace, R).  R as for goi_raster_backward.  Reads only P, S, W, H, semantics and bg from `scene`.  What it cannot
 * check is the premise: the caller vouches that nothing but the semantics changed (goi_hyperplane_amd: opt-in geometry cache,
 * DESIGN.md 7c).  No counterpart in the reference, which redoes the whole frame (CR/rasterizer_impl.cu:198-344). */
int goi_raster_forward_reblend(const GoiRasterScene* scene, int R, const void* geom_buffer, const void* binning_buffer,
                               const void* cached_image_buffer, void* image_buffer, float* out_color, float* out_semantic,
                               float* out_depth, float* out_alpha, void* stream);

/* Backward of the forward that filled the three workspaces.  R = the instance count the binning workspace was laid out
 * for: goi_raster_forward's return value, or the `capacity` of a goi_raster_forward_async frame (the kernels read the
 * true count from the geometry workspace), or num_rendered after goi_raster_forward_redo.
 * Any of the four upstream gradients dL_dout_* may be NULL (= zero).  dL_dconic is [P,4] (x: a, y: b, z: unused, w: c), dL_dsh [P,M,3] (may be NULL when M == 0).
 * dL_dconic and dL_ddepth are WORKSPACES (CR/backward.cu hands them from its render pass to its preprocess pass; no caller of
 * the reference reads them): with a scratch buffer and option "bwd_records" 1 (the default) the blend gradients travel
 * between the two passes inside the scratch instead and these two arrays are left unwritten.
 * FACTORED mode: dL_dsh == NULL while the scene has SH colours.  dL/dSH is not formed (192 of the 300 bytes of
 * gradient per Gaussian at degree 3); dL_dcolor returns the colour gradient with the forward's clamp mask applied
 * (CR/backward.cu:44-47), the factor g of dL/dSH[k] = basis_k(view direction) * g -- see goi_raster_sh_grad_from_views.
 *
 * scratch: goi_raster_backward_scratch_bytes(scratch_instances ? scratch_instances : R, S) bytes, uninitialised; NULL selects the
 * float-atomic accumulation path (not bit-reproducible).
 *
 * scratch_instances (0 = R): the row scratch laid out for FEWER instances than the binning workspace.  `R` stays what the
 * binning buffer was laid out for (a speculative frame: its capacity); `scratch_instances` is what the scratch --
 * goi_raster_backward_scratch_bytes(scratch_instances, S) bytes -- holds rows for.  It must be >= the frame's num_rendered: a
 * caller that has READ the count of a speculative frame by the time it enqueues the backward (the loss usually sits in between)
 * passes the count and needs half the scratch of a frame sized by its capacity (headroom 2: 2.1 instead of 4.3 GB on the
 * headline view, 6.4 instead of 12.9 GB at 3 M Gaussians).  Same results bit for bit.
 *
 * flags: bit 0, GOI_BACKWARD_ACCUMULATE: the eleven output arrays already hold the gradients of earlier views of the same batch
 * (written by a call without the bit, then possibly added to by calls with it) and this view's gradients are ADDED: the rows of a
 * Gaussian that is visible in this view are read, added to and written back, all other rows are left alone -- the sum over the K
 * views of a batch costs each view its visible rows once more instead of a dense [P, 75 + S] addition per view.  Default (record)
 * path with dL_dsh formed or no SH at all; prev_radii, prev_mask and row_mask must be NULL (an idle Gaussian then costs nothing
 * at all).  (Not in the reference: its loop back-propagates one view per optimiser step, train.py:96-198; dist.backward_views
 * uses it for multi-view batches.)
 *
 * prev_radii (or NULL): the radii array of the backward that LAST WROTE these very output buffers -- all eleven of them, e.g.
 * views of one allocation a binding keeps and reuses once its consumers have let go of it -- provided nothing else has written to
 * them since.  A Gaussian with prev_radii == 0 that is invisible in this frame as well already has zeros in every output row, and
 * nothing is written for it: on the headline scene half of the Gaussians are invisible in any one view and the dense gradient
 * tensors of the reference's interface (rasterize_points.cu:252-262: eleven zero-filled [P, ..] tensors per call) are 170 MB of
 * zeros per step.  The results are those of a call with prev_radii == NULL bit for bit.  (Honoured on the default path -- row
 * records; the other backward variants write every row.)  csrc/torch_binding.cpp keeps such a pool and checks refcount and
 * version counter before a reuse.
 *
 * prev_mask, row_mask: a per-ROW record of what a backward left in the eleven output arrays.  On the default path (row records,
 * option bwd_skip_idle 1) the per-Gaussian chain runs only for a Gaussian that reached a pixel: the row reduction publishes one
 * CONTRIBUTION byte per listed Gaussian ("owns at least one valid row") in the scratch, and a visible Gaussian whose byte is 0 --
 * it sits behind the saturation front in every tile it touches -- or that has no tiles is handled like an invisible one: its rows
 * get zeros.  On a scene with depth complexity that is two thirds of the visible Gaussians.  "The row already holds zeros" can
 * then no longer be told from a radii array, so:
 *   row_mask  [P] bytes, written (or NULL): 1 -- this call's chain wrote the row of that Gaussian, 0 -- the row holds zeros now;
 *   prev_mask [P] bytes, read (or NULL): the row_mask of the backward that LAST WROTE these very output buffers, nothing else
 *             having written to them since: a row with prev_mask 0 that gets zeros again is not written.  Takes precedence over
 *             prev_radii, which keeps its meaning.  prev_mask and row_mask may be the same array.
 * The gradients are those of bwd_skip_idle 0 under IEEE equality: the chain on an all-zero record could write -0.0 where the zero
 * path writes +0.0; the blend-gradient arrays are bit-identical.  csrc/torch_binding.cpp keeps the mask with its pooled buffer. */
#define GOI_BACKWARD_ACCUMULATE 1
int goi_raster_backward(const GoiRasterScene* scene, int R, int scratch_instances, int flags,
                        const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                        const int* radii, const float* out_alpha,
                        const float* dL_dout_color, const float* dL_dout_semantic,
                        const float* dL_dout_depth, const float* dL_dout_alpha,
                        float* dL_dmean2D /*[P,3]*/, float* dL_dconic /*[P,4]*/, float* dL_dopacity /*[P]*/,
                        float* dL_dcolor /*[P,3]*/, float* dL_dsemantic /*[P,S]*/, float* dL_ddepth /*[P]*/,
                        float* dL_dmean3D /*[P,3]*/, float* dL_dcov3D /*[P,6]*/, float* dL_dsh /*[P,M,3]*/,
                        float* dL_dscale /*[P,3]*/, float* dL_drot /*[P,4]*/,
                        void* scratch, const int* prev_radii, const uint8_t* prev_mask, uint8_t* row_mask, void* stream);

/* Tests only: byte offset, in a 256-byte aligned scratch of goi_raster_backward_scratch_bytes(num_rendered, S), of the contribution
 * bytes the default backward leaves there: [num_rendered] bytes indexed by a listed Gaussian's first emit-order instance (word 0 of
 * its aux entry), 1 = the Gaussian owns at least one valid row.  Written for every listed Gaussian of a frame that is not truncated;
 * every other byte keeps what the caller left there. */
size_t goi_raster_debug_backward_contrib_offset(int num_rendered, int S);

/* Feature-gradient-only backward: dL/dsemantics [P,S] from dL/d(semantic map) alone, bit-identical to
 * the dL_dsemantic of goi_raster_backward and about 3x cheaper.  For the reference's default training
 * configuration, where only the semantic features are optimised (arguments/__init__.py:85-90,
 * scene/gaussian_model.py:185-246).  Same workspaces, `R` and scratch as goi_raster_backward. */
int goi_raster_backward_semantics(const GoiRasterScene* scene, int R, const void* geom_buffer,
                                  const void* binning_buffer, const void* image_buffer, const int* radii,
                                  const float* out_alpha, const float* dL_dout_semantic, float* dL_dsemantic,
                                  void* scratch, void* stream);

/* Trace: scene->semantics is ignored; img_sem[S,H,W] is scattered onto the Gaussians it meets
 * with alpha > 0.005.  out_color[3,H,W], gau_sem[P,S], num_gsem[P] (int32), radii[P]. */
int goi_raster_trace(const GoiRasterScene* scene, const float* img_sem, void* geom_buffer, void* image_buffer,
                     goi_alloc_fn binning_alloc, void* alloc_user,
                     float* out_color, float* gau_sem, int* num_gsem, int* radii, void* stream);

/* present[P] (bytes, 0/1): view-space z > 0.2. */
int goi_raster_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                            uint8_t* present, void* stream);

/* ---- semantic head, inference decode ----------------------------------------
 * Replaces, per pixel, gui/main.py:364-386 of the reference with scene/semantic_model.py used as one
 * Linear(S -> n_codes, bias):  idx = argmax_c (W[c,:] . f + b[c]);  sim = code_score[idx];
 * sim < thresh -> background (sim = 0).  `sem` is the rasterizer's semantic output [S, HW]
 * (channel-major, no permute); W is [n_codes, S] row-major (torch Linear.weight); code_score[n_codes]
 * is the host-folded tail (LUT lookup -> L2 normalise -> LinearSVM/VLM score).  Any of sim_out[HW],
 * idx_out[HW] (int32), bg_mask_out[HW] (bytes) may be NULL.  Ties go to the lowest code index.
 * 1 <= S <= 32 and 1 <= n_codes <= 16 * floor(10240 / (16 * ceil(S / 4) + 4)) (the code book staged in 160 KiB of LDS:
 * 8192 codes at S <= 4, 2400 at S = 13..16, 1232 at S = 29..32); a larger code book is refused with nothing written.
 * Which kernel serves a call (csrc/semantic_head.hip): S <= 16 and n_codes <= 576 (64 KiB of LDS) under "decode_variant"
 * 1 .. 3 the split-bf16 contraction semantic_decode3n_k; every other shape, and every shape under decode_variant 0, the
 * fp32-MFMA semantic_decode_k (specialised for 289..304 codes at S = 13..16).  Both are accurate to fp32 rounding of
 * the logits. */
int goi_semantic_decode(const float* sem, int S, long long HW, const float* W, const float* bias, int n_codes,
                        const float* code_score, float thresh, float* sim_out, int* idx_out, uint8_t* bg_mask_out,
                        void* stream);

/* ---- semantic-space hyperplane fine-tune (gui/main.py:1673-1763, finetune_prompt_with_res; csrc/osh.hip) -------------
 * The reference trains its LinearSVM (networks.py:12-59: o = w . (x / 0.3438) + b) with hinge loss and SGD against a binary
 * mask, one epoch per step, until IoU >= target_iou or max_epochs.  Every pixel's feature is a normalised code-book row, so
 * the fit depends on the frame only through two histograms over the decoded codes.
 *
 * goi_semantic_osh_counts ADDS into counts [2][n_codes] (int32, the caller zeroes it): row 0 the pixels with idx = c and
 * positive != 0, row 1 those with positive == 0.  idx [HW] (int32: goi_semantic_decode's idx_out), positive [HW] (bytes).
 * Codes outside [0, n_codes) are not counted.  1 <= n_codes <= 1000.
 *
 * goi_semantic_osh_fit runs K independent fits in one launch (one workgroup each), all epochs on the device:
 *   lut [n_codes][D] fp32 (z_c = (lut[c] / |lut[c]|) / 0.3438), counts [K][2][n_codes] (as above), HW = pixels per frame
 *   (the mean's divisor), w [K][D] and b [K] (in: initial hyperplane, out: fitted), lr (SGD), max_epochs (1 .. 1e6),
 *   target_iou (stop after the first epoch whose IoU is not below it; a NaN IoU also stops).
 *   Writes, per fit: epochs_out (epochs run, >= 1; -1 if a code present in counts has an all-zero LUT row, and then w / b
 *   are left as they were), loss_out (the last epoch's loss, taken before its step), iou_out (IoU after the last step,
 *   double, NaN for an empty union), init_iou_out (IoU of the initial hyperplane); trace (NULL or [K][max_epochs][2]
 *   doubles): (loss, IoU) of every epoch run.  1 <= D <= 1024, 1 <= n_codes <= 1000, 1 <= HW < 2^31. */
#define GOI_OSH_MAX_EPOCHS 1000000
int goi_semantic_osh_counts(const int* idx, const uint8_t* positive, long long HW, int n_codes, int* counts, void* stream);
int goi_semantic_osh_fit(const float* lut, int n_codes, int D, const int* counts, long long HW, int K, float* w, float* b,
                         float lr, int max_epochs, double target_iou, int* epochs_out, float* loss_out, double* iou_out,
                         double* init_iou_out, double* trace, void* stream);

/* ---- exact DBSCAN of a point set (gui/main.py:1595-1665 runs sklearn.cluster.DBSCAN(eps=0.35, min_samples=600) on the
 * selected Gaussians' positions; csrc/dbscan.hip).  labels [n] (int32) equal sklearn's DBSCAN(eps, min_samples).fit(X).labels_
 * for the neighbour test d2 <= eps*eps evaluated in fp32 as dx = xi - xj (y, z alike), d2 = fma(dz,dz, fma(dy,dy, dx*dx)):
 * core points have >= min_samples neighbours (themselves included), clusters are the connected components of the core points
 * numbered by their smallest core index, a border point takes the smallest label among its core neighbours, noise is -1.
 * core [n] (bytes, may be NULL) receives the core flags.  result (device, 2 ints): result[0] = number of clusters,
 * result[1] = DBSCAN_FLAG_* bits; when result[1] != 0 the labels are not to be used.  points [n][3] fp32, device.
 * workspace: goi_semantic_dbscan_workspace_bytes(n) bytes of device memory, 256-byte aligned.  Asynchronous on `stream`, no
 * host read-back; bit-identical from run to run.  Returns < 0 (goi_raster_last_error) for eps <= 0 or non-finite,
 * min_samples < 1, n < 0 or n >= 2^30 (the radix sort of the cell keys is exact below 2^30 keys); eps outside [2^-40, 2^40] (where the grid's exactness argument stops) is reported
 * as DBSCAN_FLAG_RANGE.  n = 0 gives 0 clusters. */
#define DBSCAN_FLAG_NONFINITE 1 /* a coordinate is NaN or infinite (sklearn raises ValueError) */
#define DBSCAN_FLAG_SORT 2      /* a radix-sort look-back ran out of its spin budget (a wedged device) */
#define DBSCAN_FLAG_RANGE 4     /* the extent needs more than 2^21 grid cells on an axis, or eps is outside [2^-40, 2^40] */
#define DBSCAN_FLAG_GRID 8      /* a grid cell failed its clique check (cannot happen inside the range; never silent) */
#define DBSCAN_FLAG_UNION 16    /* a union-find loop reached its bound (cannot happen; never silent) */
size_t goi_semantic_dbscan_workspace_bytes(long long n);
int goi_semantic_dbscan(long long n, const float* points, float eps, int min_samples, int* labels, uint8_t* core, int* result,
                        void* workspace, void* stream);

/* ---- bit-packed binary masks of a camera sweep (csrc/masks.hip): the mask stage of the relevant-camera precompute
 * (gui/main.py:407-478: torch.count_nonzero(cos_sim), cos_sim > 0, cv2.dilate(mask, ones((3,3)), iterations=5) >= 0.5 on
 * the host) and of the segmentation evaluation (gui/main.py:1957-2016 with utils/image_utils.py:59-102).
 * A packed mask buffer is [V][H][Wwords] uint64, Wwords = ceil(W / 64): bit j of word w of row y is pixel (y, 64 w + j);
 * bits past W are zero.  Every call is asynchronous on `stream`: no allocation, copy or synchronisation.  Returns < 0
 * (goi_raster_last_error) for bad sizes or NULL pointers; pointers are device memory; H * W < 2^31.
 *
 * goi_semantic_mask_pack packs n_views maps src [n_views][H][W] (GOI_MASK_F32: bit = x > 0, a NaN clears it;
 *   GOI_MASK_U8: bit = x != 0) into views first_view .. first_view + n_views - 1 of `packed`.  counts (NULL or [V][2]
 *   int64) is ADDED to (the caller zeroes it): counts[v][0] += pixels with x != 0 (count_nonzero: a NaN counts),
 *   counts[v][1] += set bits.  1 <= n_views <= 65535.
 * goi_semantic_mask_dilate: dst = src dilated by the square of radius `radius` clipped at the border (cv2.dilate with
 *   ones((k,k)) and n iterations is radius n(k-1)/2; its default border never contributes).  0 <= radius <=
 *   GOI_MASK_MAX_RADIUS, dst != src.
 * goi_semantic_mask_unpack: out [n_out][H][W] bytes (0 / 1) from views index[0 .. n_out-1] of the n_views views of
 *   packed (index NULL: views 0 .. n_out-1); an index outside 0 .. n_views-1 gives an all-zero mask.
 * goi_semantic_mask_confusion: out [n_views][4] int64 = TP, FP, FN, TN of pred against gt per view (one workgroup per
 *   view, deterministic). */
#define GOI_MASK_F32 0
#define GOI_MASK_U8 1
#define GOI_MASK_MAX_RADIUS 63
int goi_semantic_mask_pack(const void* src, int src_dtype, int n_views, int H, int W, int first_view, uint64_t* packed, long long* counts,
                  void* stream);
int goi_semantic_mask_dilate(const uint64_t* src, uint64_t* dst, int n_views, int H, int W, int radius, void* stream);
int goi_semantic_mask_unpack(const uint64_t* packed, int n_views, int H, int W, int n_out, const long long* index, uint8_t* out,
                             void* stream);
int goi_semantic_mask_confusion(const uint64_t* pred, const uint64_t* gt, int n_views, int H, int W, long long* out, void* stream);

/* ---- the viewer's frame (csrc/display.hip): the stage between a render with its decoded similarity and the displayed
 * picture, which the reference runs on the host in numpy (gui/main.py:549-604 test_step, :387-398 set_clip_mask with
 * utils/image_utils.py:129-178 cmap / clip_color, :1766-1801 render_video).
 *
 * goi_semantic_frame_compose: out [n_views][H][W][3] (GOI_FRAME_F32 or GOI_FRAME_U8, interleaved) from base [n_views]
 *   [channels][H][W] fp32 (channels 1 or 3; 1 is repeated to three), sim [n_views][H][W] fp32 and bg_mask [n_views][H][W]
 *   bytes (nonzero = background).  Every operation is one fp32 rounding, in this order:
 *     normalize != 0: base = (base - min_v) / ((max_v - min_v) + 1e-20f), min / max over the whole view; then
 *     base = clamp(base, 0, 1);
 *     GOI_FRAME_NONE     out = base
 *     GOI_FRAME_BINARY   out = sim > 0 ? 1 : 0                                   (base is not read)
 *     GOI_FRAME_WHITEN   col = 1; opa = (bg ? 1 : 0) * r; om = 1 - opa
 *     GOI_FRAME_HEAT     rel = clamp(((sim - t) - 0.05f) / (max_v(sim) - t), 0, 1); col = bg ? 1 : clamp(table[(long)(rel *
 *                        (n_colors - 1))], 0, 1); opa = r; om = (float)(1.0 - overlay_ratio), the subtraction in double
 *     GOI_FRAME_HEAT_FT  rel = clamp(sim + 0.2f, 0.1f, 0.9f); col as HEAT; opa = (bg ? 1 : 0) * r; om = 1 - opa
 *     the three overlay styles: out = clamp(col * opa + base * om, 0, 1), never contracted to an FMA;
 *     GOI_FRAME_U8: out = (uint8)(out * 255f), truncated.
 *   r = (float)overlay_ratio, t = (float)heat_thresh.  sim is needed by BINARY, HEAT and HEAT_FT, bg_mask by WHITEN, HEAT
 *   and HEAT_FT, table [n_colors][3] fp32 (2 <= n_colors <= GOI_FRAME_MAX_COLORS) by HEAT and HEAT_FT; the others may be
 *   NULL.  The table index is clamped into the table and a NaN rel takes entry 0; the minima and maxima skip NaNs; the
 *   sign of a zero in `out` is unspecified.  workspace: goi_semantic_frame_workspace_bytes(n_views) bytes of device
 *   memory, 4-byte aligned, zeroed on `stream` by the call when it is used (normalize, or GOI_FRAME_HEAT).
 *   At most two kernel launches whatever n_views is, asynchronous on `stream`: no allocation, copy or synchronisation.
 *   16-byte aligned buffers with H * W a multiple of 4 take the vector path; anything else a scalar one with the same
 *   result.  1 <= n_views <= 65535, H * W < 2^31.  Returns < 0 (goi_raster_last_error) for bad arguments. */
#define GOI_FRAME_NONE 0
#define GOI_FRAME_BINARY 1
#define GOI_FRAME_WHITEN 2
#define GOI_FRAME_HEAT 3
#define GOI_FRAME_HEAT_FT 4
#define GOI_FRAME_F32 0
#define GOI_FRAME_U8 1
#define GOI_FRAME_MAX_COLORS 1024 /* the table is staged in LDS: 12 KiB */
size_t goi_semantic_frame_workspace_bytes(int n_views);
int goi_semantic_frame_compose(const float* base, int channels, const float* sim, const uint8_t* bg_mask, int n_views, int H, int W,
                               int style, int normalize, double overlay_ratio, double heat_thresh, const float* table,
                               int n_colors, void* out, int out_dtype, void* workspace, void* stream);

/* ---- a PCA picture of the semantic features (csrc/pca.hip): three principal components of the S-dimensional feature
 * field as a colour, which the reference computes on the host (gui/main_edit.py:1841-1870 visual_latent with
 * utils/visual_latent.py:32-40: the rendered map copied to the host and sklearn's PCA(n_components=3).fit_transform).
 * Samples come in one of two layouts, GOI_PCA_PLANAR [S][n] (a rendered map, read in place) or GOI_PCA_ROWS [n][S] (the
 * Gaussians' own features); 3 <= S <= 32, 1 <= n < 2^31.
 *
 * goi_semantic_pca_accumulate: adds the count, the per-channel sums and the S x S second moments of x's samples to
 *   `workspace` (goi_semantic_pca_workspace_bytes(S, 0) bytes of device memory, 256-byte aligned).  mask: NULL, or n
 *   bytes, nonzero = use the sample; a sample that is not used is never read into the sums (it may hold a NaN).
 *   first != 0 starts a fit: it fixes the pivot c (the channel means of the used samples among 2048 samples, in chunks of
 *   32 spread evenly over the whole set, so a map whose first rows are empty background still gets its foreground's mean; of all of
 *   these when none is used; 0 where that is not finite) and overwrites the workspace; first == 0 adds to it, which
 *   is how a camera set is fitted.  The sums are of (x - c) and (x - c)(x - c)^T, so features far from zero lose
 *   nothing; fp32 inside a wave (the Gram update is v_mfma_f32_16x16x4_f32, an exact fmaf chain), fp64 across waves,
 *   workgroups and calls, in a fixed order: no float atomics, the result is bit-reproducible.
 * goi_semantic_pca_solve: the basis of what was accumulated, GOI_PCA_BASIS_FLOATS(S) fp32 at `basis`:
 *     mean[S]; components[3][S]; explained_variance[3]; total_variance; count
 *   in fp64: mean = c + sum / n, covariance with divisor n - 1 (the pivot cancels exactly), cyclic Jacobi with a fixed
 *   maximum of 16 sweeps, the three largest eigenpairs in descending order, the entry of largest magnitude of each
 *   component positive (sklearn >= 1.5: svd_flip(u_based_decision=False)), negative eigenvalues clipped to 0:
 *   sklearn.decomposition.PCA(3)'s mean_, components_, explained_variance_.  total_variance is the trace of the
 *   covariance.  count is rounded to fp32 (exact below 2^24).  Fewer than two used samples: components and variances
 *   are 0, the mean is that of what there was, nothing is NaN.  Non-finite input gives a non-finite basis, never a hang.
 * goi_semantic_pca_apply: q_k = sum_c (x_c - mean_c) * component_k[c], c ascending, every operation one fp32 rounding
 *   (no FMA), for each sample of n_views views x [n_views][S][n] or [n_views][n][S]; out [n_views][3][n]
 *   (GOI_PCA_PLANAR: a `base` of goi_semantic_frame_compose) or [n_views][n][3] (GOI_PCA_ROWS: a colors_precomp).
 *     GOI_PCA_RAW     out = q                                                     (PCA.fit_transform / transform)
 *     GOI_PCA_SIGMA   out = clamp(0.5f + q / ((2 k) * max(sqrtf(explained_variance_k), FLT_MIN)), 0, 1), k = (float)k_sigma;
 *                     a NaN q gives 0.  The scale is the basis's, so colours are stable from frame to frame; k is a
 *                     display choice (2.0: +-2 sigma span the range)
 *     GOI_PCA_MINMAX  out = (q - min) / ((max - min) + 1e-20f), min / max per view and component, NaNs skipped
 *   q is computed by the same code in every mode, layout and path.  workspace: needed by GOI_PCA_MINMAX only,
 *   goi_semantic_pca_workspace_bytes(0, n_views) bytes, 4-byte aligned, zeroed by the call with one hipMemsetAsync on
 *   `stream`.  At most two kernel launches (plus that memset for GOI_PCA_MINMAX) whatever n_views is.  Planar input with n % 4 == 0 and x, out on 16-byte boundaries takes 16-byte
 *   loads and stores; anything else one sample per thread, with the same bits.  0 <= n_views <= 65535 (0: nothing is
 *   done, 0 is returned).
 * goi_semantic_pca_workspace_bytes(S, n_views): the bytes a fit of S channels needs (S > 0) plus those a MINMAX apply of
 *   n_views views needs (n_views > 0); 0 for arguments out of range.
 * All three are asynchronous on `stream`: no allocation, copy or synchronisation.  They return < 0
 * (goi_raster_last_error) for bad arguments. */
#define GOI_PCA_PLANAR 0
#define GOI_PCA_ROWS 1
#define GOI_PCA_RAW 0
#define GOI_PCA_SIGMA 1
#define GOI_PCA_MINMAX 2
#define GOI_PCA_MIN_DIM 3
#define GOI_PCA_MAX_DIM 32
#define GOI_PCA_BASIS_FLOATS(S) (4 * (S) + 5)
size_t goi_semantic_pca_workspace_bytes(int S, int n_views);
int goi_semantic_pca_accumulate(const float* x, int layout, int S, long long n, const uint8_t* mask, int first, void* workspace,
                                void* stream);
int goi_semantic_pca_solve(int S, void* workspace, float* basis, void* stream);
int goi_semantic_pca_apply(const float* x, int in_layout, int S, long long n, int n_views, const float* basis, int normalize,
                           double k_sigma, float* out, int out_layout, void* workspace, void* stream);

/* ---- code-book initialisation (train.py:78-86; csrc/codebook_init.hip) ----------------------------------------------
 * goi_codebook_unique_rows: the rows of x.permute(1, 2, 0).reshape(-1, D).unique(dim=0) of each of n_views fp32 maps
 *   maps[v] [D][H][W] (a host array of n_views device pointers; the maps are read in place), exact: rows are compared by
 *   value (-0 == +0; the kept row is the first pixel's), written in ascending lexicographic order of their values.
 *   The call synchronises `stream` once to read the per-view counts, then asks alloc(alloc_user, bytes) for the output
 *   [sum counts][D] fp32 (views one after another) and fills it asynchronously; a view of more than
 *   GOI_CODEBOOK_RANK_MAX distinct rows (or of D > 8192) is sorted by D radix sorts, after which the call synchronises once more to read
 *   the sort's error bit.  counts (host, [n_views]) and flags (host, GOI_CODEBOOK_FLAG_* bits) are written; when
 *   *flags != 0 nothing is allocated or written and the rows are not to be used.  1 <= D, H * W < 2^30.
 *   workspace: goi_codebook_unique_rows_workspace_bytes(n_views, D, H, W) bytes of device memory, 256-byte aligned.
 * goi_codebook_kmeans: spherical k-means (train.py:36-56) of n_problems problems at once.  Problem p owns rows
 *   row_offsets[p] .. row_offsets[p+1]-1 (device, int64) of x [n_rows][D] fp32, which is normalised IN PLACE (a zero
 *   row becomes NaN, as in the reference); max_rows = the largest problem's row count (host).  perms (device, int32)
 *   holds, per problem from (niter + 1) * row_offsets[p] on, the niter + 1 permutations of 0 .. N_p-1 the reference
 *   draws (torch.randperm(N_p): the seed order, then one per iteration).  centers [n_problems][ncluster][D] receives
 *   the final centres (the last means with dead centres replaced, not normalised).  status (device, [n_problems]
 *   int32): 0, or 1 + the iteration at which more centres died than the problem has rows (the reference raises
 *   there).  fp32 throughout, no float atomics: bit-identical from run to run.  Asynchronous: no host synchronisation.
 *   Every problem needs N_p >= 1.  1 <= ncluster <= GOI_CODEBOOK_KMEANS_MAX_K, 1 <= D <= GOI_CODEBOOK_KMEANS_MAX_DIM.
 *   workspace: goi_codebook_kmeans_workspace_bytes(n_rows, n_problems, ncluster, D) bytes, 256-byte aligned. */
#define GOI_CODEBOOK_FLAG_NONFINITE 1 /* a map holds a NaN or an Inf (the reference's order is undefined there) */
#define GOI_CODEBOOK_FLAG_SORT 2      /* a radix-sort look-back ran out of its spin budget (a wedged device) */
#define GOI_CODEBOOK_FLAG_TABLE 4     /* a hash probe reached its bound (cannot happen: the table is twice the pixels) */
#define GOI_CODEBOOK_RANK_MAX 4096
#define GOI_CODEBOOK_KMEANS_MAX_K 4096
#define GOI_CODEBOOK_KMEANS_MAX_DIM 1024
size_t goi_codebook_unique_rows_workspace_bytes(int n_views, int D, int H, int W);
int goi_codebook_unique_rows(const float* const* maps, int n_views, int D, int H, int W, long long* counts, unsigned* flags,
                             goi_alloc_fn alloc, void* alloc_user, void* workspace, void* stream);
size_t goi_codebook_kmeans_workspace_bytes(long long n_rows, int n_problems, int ncluster, int D);
int goi_codebook_kmeans(float* x, const long long* row_offsets, int n_problems, long long max_rows, long long n_rows, int D,
                        int ncluster, int niter, const int* perms, float* centers, int* status, void* workspace, void* stream);

/* ---- photometric loss and image metrics (train.py:137-140, utils/loss_utils.py, utils/image_utils.psnr; csrc/photometric.hip)
 * img1, img2: [n][c][h][w] fp32 (a [c][h][w] image is n = 1).  SSIM is loss_utils._ssim: the 11x11 Gaussian window
 *   (sigma 1.5), zero padding of 5 per (image, channel) plane, C1 = 0.01^2, C2 = 0.03^2.  window_size must be
 *   GOI_PHOTOMETRIC_WINDOW; other sizes are refused.  1 <= h, w; h * w < 2^31; n * c * ceil(h/32) * ceil(w/32) < 2^31.
 * goi_raster_photometric_forward: out (device, [3]) = loss = (1 - lambda_dssim) * L1 + lambda_dssim * (1 - SSIM), L1 = mean |img1 -
 *   img2|, SSIM = mean of the SSIM map, all over every element.  out_images (device, [3][n], or NULL) = per image the SSIM
 *   mean, the L1 mean and PSNR = 20 log10(1 / sqrt(mean (img1 - img2)^2)).  flags GOI_PHOTOMETRIC_GRAD1 / _GRAD2 keep in
 *   the workspace what the backward needs for the gradient of img1 / img2.
 * goi_raster_photometric_backward: after a forward with the same arguments, flags and workspace (untouched in between): grad1 =
 *   dL/dimg1 (GRAD1), grad2 = dL/dimg2 (GRAD2), for L = the loss above (flags without GOI_PHOTOMETRIC_SSIM_ONLY) or the SSIM
 *   mean itself (with it), times the upstream gradient grad_out (device): one value for the mean over every element, or
 *   with GOI_PHOTOMETRIC_PER_IMAGE one value per image for per-image means.  The L1 term's gradient is 0 where img1 == img2.
 *   workspace: goi_raster_photometric_workspace_bytes(n, c, h, w, flags) bytes of device memory, 256-byte aligned.
 * Sums are formed in a fixed order without float atomics: bit-identical from call to call.  No host synchronisation. */
#define GOI_PHOTOMETRIC_WINDOW 11
#define GOI_PHOTOMETRIC_GRAD1 1u     /* the gradient of img1 is wanted */
#define GOI_PHOTOMETRIC_GRAD2 2u     /* the gradient of img2 is wanted */
#define GOI_PHOTOMETRIC_PER_IMAGE 4u /* backward: grad_out holds n values, of per-image means */
#define GOI_PHOTOMETRIC_SSIM_ONLY 8u /* backward: the gradient of the SSIM mean, not of the loss */
size_t goi_raster_photometric_workspace_bytes(long long n, int c, int h, int w, unsigned flags);
int goi_raster_photometric_forward(const float* img1, const float* img2, long long n, int c, int h, int w, int window_size,
                                   float lambda_dssim, unsigned flags, float* out, float* out_images, void* workspace, void* stream);
int goi_raster_photometric_backward(const float* img1, const float* img2, long long n, int c, int h, int w, int window_size,
                                    float lambda_dssim, unsigned flags, const float* grad_out, const void* workspace, float* grad1,
                                    float* grad2, void* stream);

/* ---- measurement hooks (bench.py): per-stage HIP-event timing on the launch stream ---------- */
enum {
    GOI_STAGE_PREPROCESS = 0,   /* forward per-Gaussian kernel */
    GOI_STAGE_DEPTH_SORT,       /* radix sort of Gaussians by depth */
    GOI_STAGE_SCAN,             /* prefix sum of tiles_touched + num_rendered read-back */
    GOI_STAGE_EMIT,             /* (tile, Gaussian) instance emission */
    GOI_STAGE_TILE_SORT,        /* stable radix sort of instances by tile */
    GOI_STAGE_RANGES,           /* per-tile [start,end) */
    GOI_STAGE_BLEND_FWD,        /* forward alpha blend */
    GOI_STAGE_BLEND_BWD,        /* backward alpha blend */
    GOI_STAGE_PREPROCESS_BWD,   /* cov2D + projection + SH + cov3D backward */
    GOI_STAGE_COUNT
};
/* on != 0: record events around every stage of subsequent calls (adds event overhead). */
void goi_raster_profile_enable(int on);
/* Same, restricted to the stages whose bit (1u << GOI_STAGE_x) is set; 0 turns profiling off.  Timing
 * one stage costs two event records per call instead of two per stage. */
void goi_raster_profile_stages(unsigned stage_mask);
/* Synchronises the recorded events and ADDS each stage's elapsed milliseconds and launch count
 * since the last reset into ms[GOI_STAGE_COUNT] / calls[GOI_STAGE_COUNT]; then resets. */
int goi_raster_profile_collect(double* ms, int* calls);

/* Tuning / experiment switches; the defaults are the shipped configuration.
 *   "fwd_variant"  1 (default) two candidates per loop trip in the forward blend, 0 one (bit-identical); other values are
 *                  refused
 *   "bwd_variant"  0 (default) atomic-free backward; the per-Gaussian sums over pixels run at the 16-bit matrix rate on
 *                  split operands that keep fp32 accuracy (two f16 planes of exactly scaled values, all four partial
 *                  products, fp32 accumulation: indistinguishable from the fp32 chain at the noise level of two builds of
 *                  the reference -- profiles/r04_flush_equivalence*.json; bit-reproducible); 2 the same with exact-fp32
 *                  MFMA (one fp32 FMA chain per output); 1 workgroup-per-tile backward with float atomics (what
 *                  scratch = NULL selects)
 *   "sort_variant" 1 (default) onesweep radix sort, 0 histogram / scan / scatter per pass
 *   "sort_lookback" 1 (default) onesweep passes of up to 640 tiles find their prefix with the GROUPED look-back (a tile adds up the
 *                  aggregates of its group, then the totals of the groups in front: two round trips), 0 always the chained
 *                  decoupled look-back; same order either way
 *   "sort_small"   0 (default) sorts of up to 2 M keys use 1024 x 4-key tiles; 1 they take the adaptive 512 x (2..16) tile that
 *                  larger sorts choose from the device-side count (slower for them: DESIGN.md 8.2); same order either way
 *   "cull_variant" 2 (default) a Gaussian is listed only in the tiles its contribution ellipse (alpha >= 1/255) reaches,
 *                  1 in the tiles its axis-aligned contribution box touches, 0 in the reference's 3-sigma squares.
 *                  Identical images; gradients equal up to the order of one fp32 sum
 *   "decode_variant" (goi_semantic_decode, S <= 16) 1 (default) contraction as three bf16 MFMAs on exact 3-way splits of
 *                  the fp32 operands (fp32 accuracy), two 16-pixel blocks per code-book operand fetch; 2 / 3 the same
 *                  with four / one block per fetch (bit-identical results, slower); 0 fp32 MFMA
 *   "bwd_order"    1 (default) the backward's quadrant waves are launched longest-first inside each XCD's band (their
 *                  cost is known from the forward; cost classes of 16 list positions), 2 .. 4 the same with classes of 32 ..
 *                  128 positions (closer to tile order: less HBM traffic, less balance), 0 in tile order; same gradients
 *   "bwd_records"  1 (default) the per-Gaussian sums of the atomic-free backward stay in the scratch as one record per
 *                  listed Gaussian and the per-Gaussian pass writes every per-id output; 0 they go through six per-id
 *                  arrays (dL_dconic, dL_ddepth, ... and zeros for the Gaussians that are not listed); same gradients, bit for bit;
 *                  2 EXPERIMENT (128-byte rows: S = 5 .. 20): the per-Gaussian pass sums its Gaussians' rows itself -- no record,
 *                  no reduce_rows_k; bit-identical, measured slower
 *   "bwd_skip_idle" (bwd_records 1) 1 (default) a visible Gaussian that reached no pixel -- no valid row in any tile it touches, or
 *                  no tiles -- skips the per-Gaussian chain and its rows get zeros (goi_raster_backward, row_mask); 0 every visible
 *                  Gaussian goes through the chain.  Equal gradients (zeros may differ in sign)
 *   "osh_path"     goi_semantic_osh_fit: 0 (default) z in registers where the shape allows it (D = 256, n_codes <= 320),
 *                  1 always the generic path (z re-formed from the LUT every epoch); bit-identical (285 -> 437 us on the headline view: DESIGN.md 9.3)
 * Thread safety: the set is changed under a mutex; an entry point snapshots it when it starts. */
int goi_raster_set_option(const char* name, int value);

/* dL/dSH [P,M,3] of V views from the factors goi_raster_backward leaves in FACTORED mode: means3D [P,3], the V camera
 * centres campos [V,3] and the clamp-masked colour gradients gcol [V,P,3]:
 *     dL_dsh[g][k] = sum_v basis_k(normalize(means3D[g] - campos[v])) * gcol[v][g]
 * with the basis of CR/backward.cu:49-109 (degree D, (D+1)^2 <= M <= 16; coefficients above (D+1)^2 get 0), views added
 * in index order: bit-identical to adding the per-view dL_dsh arrays of goi_raster_backward in that order.  Lets a
 * data-parallel job exchange 12 bytes per Gaussian and view (all-gather) instead of all-reducing 192. */
int goi_raster_sh_grad_from_views(int P, int D, int M, int V, const float* means3D, const float* campos, const float* gcol,
                           float* dL_dsh, void* stream);

/* ---- simple_knn._C.distCUDA2 (submodules/simple-knn/ext.cpp:15-17, spatial.cu:15-26,
 * simple_knn.cu:170-221): mean squared distance of every point to its 3 nearest OTHER points,
 * mean_dist2[i] = (d0 + d1 + d2) / 3 in fp32.  points [P,3] and mean_dist2 [P] are device pointers;
 * workspace holds goi_knn_workspace_bytes(P) bytes of device memory (256-byte aligned).  With fewer
 * than 4 points the missing neighbours count as FLT_MAX, as in the reference.  Asynchronous on
 * `stream`; no host read-back.  P >= 2^30 is refused (returns < 0; the workspace size is 0): the
 * radix sort of the Morton codes is exact below 2^30 keys. */
size_t goi_knn_workspace_bytes(int P);
int goi_knn_dist2(int P, const float* points, float* mean_dist2, void* workspace, void* stream);

/* ---- exact k-NN graph (csrc/knn.hip; the reference has no counterpart).  queries [Pq,3], refs [Pr,3] fp32;
 * query_keep [Pq] / ref_keep [Pr]: one byte per point, non-zero = in, NULL = all.  With
 *     dist2(i, j) = fmaf(dz, dz, fmaf(dx, dx, dy * dy)),  d = refs[j] - queries[i]  in fp32
 * row i of idx [Pq,k] (int32) / dist2 [Pq,k] holds the k smallest (dist2, j) pairs over the kept references in ascending
 * lexicographic order: ties in distance go to the lower j.  Nothing else enters the result: not the boxes, the visiting order
 * or the order of the input.  Ids are the caller's.  A masked-out reference is never a neighbour; the row of a masked-out query,
 * and the tail of a row with fewer than k kept references, is idx = -1, dist2 = +inf.  exclude_self = 1 skips reference j == i
 * (by id: whatever the two masks are) and is refused unless queries == refs and Pq == Pr.  1 <= k <= 16; Pq, Pr < 2^30 (the workspace size is 0 beyond).
 * workspace: goi_knn_graph_workspace_bytes(Pq, Pr) bytes of device memory, 256-byte aligned.  Asynchronous on `stream`; no host
 * read-back: the kept counts stay on the device. */
size_t goi_knn_graph_workspace_bytes(int Pq, int Pr);
int goi_knn_graph(int Pq, const float* queries, const uint8_t* query_keep, int Pr, const float* refs, const uint8_t* ref_keep,
                  int k, int exclude_self, int32_t* idx /*[Pq,k]*/, float* dist2 /*[Pq,k]*/, void* workspace, void* stream);
/* A label per row of such a graph from its neighbours' labels [Pr] (int64): an entry counts with 0 <= idx < Pr, labels[idx] >= 0
 * and dist2 <= max_dist2 (+inf allowed; dist2 == NULL: no cut).  label_out [Pq] = the label most entries carry, the LOWEST
 * among equals (the rule of contrib.assign), count_out [Pq] (int32) its count; -1 and 0 for a row without an entry.  Labels are
 * compared as values: any int64 >= 0, no histogram, no limit on the number of classes; integer arithmetic only.  k >= 1. */
int goi_knn_majority(int Pq, int k, const int32_t* idx, const float* dist2, float max_dist2, int Pr, const int64_t* labels,
                     int64_t* label_out, int32_t* count_out, void* stream);

/* ---- Neighbour consistency of per-Gaussian features on such a graph (csrc/smooth.hip) ----------------
 * f [P,S] fp32, 1 <= S <= 32; idx [P,k] int32 as goi_knn_graph returns it, k >= 1, P * k < 2^30; weight [P,k] fp32 or NULL (= 1);
 * rows [P] bytes or NULL (= all).  Entry (i, m) is an EDGE iff 0 <= idx[i,m] < P (goi_knn_majority's rule: -1 tails and ids out
 * of range are skipped) and the edge COUNTS iff rows[i] != 0; N_E is the number of counting edges (a self edge counts and adds
 * zero).  With j = idx[i,m]:
 *     L        = (1 / N_E) sum_{counting (i,m)} w[i,m] sum_c (f[i,c] - f[j,c])^2                       (0 when N_E = 0)
 *     dL/df[a] = (2 / N_E) [ sum_{m: (a,m) counts} w[a,m] (f[a] - f[idx[a,m]])  +  sum_{(i,m) counts, idx[i,m] = a} w[i,m] (f[a] - f[i]) ]
 * The second sum runs over the TRANSPOSE of the graph, which makes the gradient a gather: no float atomics, the same bits on
 * every call.
 *
 * goi_knn_transpose: from ALL edges (it knows neither rows nor weight: one transpose serves a run that redraws rows every
 *   iteration).  in_ptr [P+1] int32, in_edge [P*k] int32: the flat edge numbers e = i * k + m in ascending (idx[e], e) order, those
 *   that point at row a in in_edge[in_ptr[a] .. in_ptr[a+1]); in_ptr[P] is the number of edges and in_edge is -1 from there on.
 *   From e the source row is e / k and the weight weight[e].  In-degrees by integer atomics, an exclusive scan, a stable radix
 *   sort over the key bits P needs (a skipped entry sorts behind every edge).  P = 0 writes in_ptr[0] = 0.
 * goi_knn_smooth_loss: *loss (fp32), *n_edges (int64) and, with grad != NULL, grad [P,S] = dL/df, all on the device; in_ptr and
 *   in_edge are read only with grad (values outside their arrays are clamped or skipped: never an access out of bounds).  Per
 *   gradient element: acc = 0; over row a's k slots in slot order, then over its in-list in stored order, for every counting
 *   edge t = f[a,c] - f[other,c], acc = acc + w * t; then acc * scale with scale = float(2.0 / N_E) formed in float64 -- every
 *   operation rounded once, no FMA.  The loss of a row: per edge q = t_c^2 (+ t_{c+16}^2) per lane c < 16, summed over the 16 lanes
 *   pairwise (offsets 8, 4, 2, 1), r = r + w * q in slot order, all fp32; rows and workgroups are summed in float64 in a fixed
 *   order and *loss = float(sum / N_E).  N_E = 0 gives exact zeros.  N_E is counted on the device before the gradient is
 *   scaled: nothing is read back.
 * goi_knn_diffuse: one Jacobi step over the out-lists: W = sum_m w[i,m] and m_c = (sum_m w[i,m] f[j,c]) / W over row i's edges
 *   in slot order (acc = acc + w * f), out[i,c] = f[i,c] + lam * (m_c - f[i,c]), one rounding per operation.  A row with
 *   fixed[i] != 0 (fixed [P] bytes or NULL), without an edge or with W == 0 is copied bit for bit.  out [P,S] must not be f.
 * Refused: P < 0, S outside 1..32, k < 1, P * k >= 2^30 (the workspace size is then 0), a NULL required pointer, a NULL or
 * misaligned workspace (goi_knn_*_workspace_bytes bytes, 256-byte aligned).  P = 0 is a valid empty call.  Asynchronous on
 * `stream`; returns 0 (or -1: goi_raster_last_error). */
size_t goi_knn_transpose_workspace_bytes(int P, int k);
int goi_knn_transpose(int P, int k, const int32_t* idx, int32_t* in_ptr /*[P+1]*/, int32_t* in_edge /*[P*k]*/, void* workspace,
                      void* stream);
size_t goi_knn_smooth_loss_workspace_bytes(int P);
int goi_knn_smooth_loss(int P, int S, int k, const float* f, const int32_t* idx, const float* weight, const uint8_t* rows,
                        const int32_t* in_ptr, const int32_t* in_edge, float* loss, long long* n_edges, float* grad /*[P,S] or NULL*/,
                        void* workspace, void* stream);
int goi_knn_diffuse(int P, int S, int k, const float* f, const int32_t* idx, const float* weight, const uint8_t* fixed, float lam,
                    float* out /*[P,S]*/, void* stream);

/* ---- Instance segmentation on such a graph (csrc/segment.hip) -----------------------------------------
 * idx [P,k] int32 as goi_knn_graph returns it, k >= 1, P * k < 2^30.
 *
 * goi_knn_segment_edges: join [P,k] bytes.  With j = idx[i,m], join[i,m] = 1 iff ALL of
 *     0 <= j < P and j != i                                  (-1 tails, ids out of range and self edges never join)
 *     rows == NULL, or rows[i] != 0 && rows[j] != 0          (rows [P] bytes)
 *     labels == NULL, or labels[i] >= 0 && labels[i] == labels[j]      (labels [P] int64)
 *     GOI_SEGMENT_MAX_DIST2 is not in flags, or dist2[i,m] <= max_dist2      (dist2 [P,k] fp32; the flag needs dist2)
 *     features == NULL, or d <= tau, where d = 0 and d = fmaf(e_c, e_c, d) for c = 0 .. S-1 in that order with
 *         e_c = features[i,c] - features[j,c] in fp32 (features [P,S], 1 <= S <= 32; S is not looked at without features).  The
 *         comparison is taken as written: a NaN d never joins, tau = +inf joins every other d.  d is symmetric in (i, j) bit for
 *         bit and does not depend on the launch geometry: one lane owns the chain.
 *     GOI_SEGMENT_MUTUAL is not in flags, or idx[j,m'] == i for some m'
 *   Refused: P < 0, k < 1, P * k >= 2^30, S outside 1..32 (with features), a NaN tau, unknown flags, GOI_SEGMENT_MAX_DIST2 without
 *   dist2 or with a NaN max_dist2, a NULL idx or join, idx / features / dist2 not 4-byte or labels not 8-byte aligned.
 *
 * goi_knn_segment_components: the connected components of the UNDIRECTED graph whose edges are the entries (i, m) with
 *   0 <= j < P, j != i, join == NULL or join[i,m] != 0, and rows == NULL or rows[i] != 0 && rows[j] != 0 -- an edge that only
 *   one endpoint lists unites both.  All outputs on the device, nothing is read back:
 *     root  [P] int32   the smallest id of the row's component; -1 where rows[i] == 0 (such a row is in no component)
 *     size  [P] int32   the number of rows of the row's component; 0 where root is -1
 *     label [P] int32   the dense rank 0 .. C-1, in ascending root, of the component among those with size >= min_size; else -1
 *     count [1] int32   C
 *     status [1] int32  GOI_SEGMENT_STATUS_* bits, 0 after a good call (the convention of GOI_MESH_STATUS_*)
 *   Union-find with the larger root hooked under the smaller (atomicCAS) and path halving (atomicMin), so every output is
 *   independent of the schedule; sizes by integer atomics, combined per wave first; ranks by an exclusive scan.
 *   Refused: P < 0, k < 1, P * k >= 2^30 (the workspace size is then 0), min_size < 1, a NULL or misaligned required pointer, a
 *   NULL or misaligned workspace (goi_knn_segment_components_workspace_bytes bytes, 256-byte aligned).
 * P = 0 is a valid empty call of either: it returns 0 and touches nothing.  Asynchronous on `stream`; returns 0 (or -1:
 * goi_raster_last_error). */
#define GOI_SEGMENT_MUTUAL 1     /* flags of goi_knn_segment_edges */
#define GOI_SEGMENT_MAX_DIST2 2
#define GOI_SEGMENT_STATUS_UNION 4 /* a union-find walk or retry loop ran out of its bound (cannot happen: parents only decrease) */
int goi_knn_segment_edges(int P, int S, int k, const int32_t* idx, const float* features, float tau, const float* dist2,
                          float max_dist2, int flags, const int64_t* labels, const uint8_t* rows, uint8_t* join /*[P,k]*/,
                          void* stream);
size_t goi_knn_segment_components_workspace_bytes(int P, int k);
int goi_knn_segment_components(int P, int k, const int32_t* idx, const uint8_t* join, const uint8_t* rows, int min_size,
                               int32_t* root, int32_t* size, int32_t* label, int32_t* count, int32_t* status, void* workspace,
                               void* stream);

/* ---- Per-instance statistics over a partition (csrc/instance.hip) ------------------------------------
 * label [P] int32 as goi_knn_segment_components writes it; K >= 0 instances.  A row is in instance label[i] iff
 * 0 <= label[i] < K; every other value (-1, a label at or above K) is "in no instance".  0 <= P < 2^30, 0 <= K < 2^30.
 *
 * goi_instance_members: the partition as lists.  member_ptr [K+1] int32, member [P] int32: the rows of instance k are
 *   member[member_ptr[k] .. member_ptr[k+1]) in ascending row id, member_ptr[K] is the number of rows in an instance, member is
 *   -1 from there on.  Counts by integer atomics, an exclusive scan, a stable radix sort over the key bits K + 1 needs.
 *   P = 0 writes member_ptr = 0 and needs no workspace.
 *
 * goi_instance_stats: every statistic of every instance in one pass over the lists.  xyz [P,3] fp32 or NULL (every position is then the origin: a caller that wants the counts alone); features [P,S] fp32 or
 *   NULL (S is then not looked at), 1 <= S <= 32; weight [P] fp32 or NULL (1); hit [P] bytes or NULL (0), eight independent
 *   flag bits.  Outputs, on the device:
 *     n [K] int32            number of members                 hits [K,8] int32     members with bit b of hit set
 *     wsum [K] fp32          W = sum w                         centroid [K,3] fp32  sum w x / W
 *     lo, hi [K,3] fp32      exact minimum / maximum of the members' positions; a NaN is skipped, -0 < +0; +inf / -inf when
 *                            there is no number
 *     cov [K,6] fp32         sum w (x-c)(x-c)^T / W: xx xy xz yy yz zz        feature [K,S] fp32 (NULL without features)  sum w f / W
 *   Float64 sums of positions relative to the instance's first member, in an order that is a fixed function of the instance's own
 *   member sequence (chunks of 256 members, four interleaved accumulators per chunk, chunk partials in ascending order: the
 *   header comment of csrc/instance.hip spells it out), one rounding to fp32 at the end; W == 0 writes 0 for centroid, cov and
 *   feature.  No float atomics, the same bits on every call.  member_ptr and member are clamped before use.
 *   K = 0 returns 0 and touches nothing; P = 0 with K > 0 writes every instance's empty values.
 * Refused by both, before any device call: P < 0, K < 0, P or K >= 2^30 (the workspace size is then 0), S outside 1..32 with
 * features, a NULL required pointer, a pointer (hit apart) that is not 4-byte aligned, a NULL or misaligned workspace
 * (goi_instance_*_workspace_bytes bytes, 256-byte aligned).  Asynchronous on `stream`; returns 0 (or -1: goi_raster_last_error). */
size_t goi_instance_members_workspace_bytes(int P, int K);
int goi_instance_members(int P, int K, const int32_t* label, int32_t* member_ptr /*[K+1]*/, int32_t* member /*[P]*/, void* workspace,
                         void* stream);
size_t goi_instance_stats_workspace_bytes(int P, int K);
int goi_instance_stats(int P, int K, int S, const int32_t* member_ptr, const int32_t* member, const float* xyz, const float* features,
                       const float* weight, const uint8_t* hit, int32_t* n, int32_t* hits, float* wsum, float* centroid, float* lo,
                       float* hi, float* cov, float* feature, void* workspace, void* stream);

/* ---- The mask-contrast loss of a feature map against one view's 2D instance masks (csrc/grouping.hip) ----
 * feat [S,H,W] fp32, channel-major as the rasterizer writes `semantics`; labels [H,W] int32; K >= 0 an upper bound on the view's
 * mask ids.  Pixel p is in mask m = labels[p] iff 0 <= m < K; every other value (-1, >= K, INT32_MIN) is ignored.
 * 1 <= S <= 32, H, W >= 1, H * W <= 2^22, 0 <= K <= 65536.  With n_m the pixels of mask m, N = sum n_m, M the masks with n_m > 0,
 * mu_m the mean feature of mask m:
 *     L_intra = sum_m a_m sum_{p in m} |f_p - mu_m|^2        a_m = 1/N (balance 0: "pixel")   1/(M n_m) (balance 1: "mask")
 *     L_inter = 1/(M(M-1)) sum_{m != m', both non-empty} max(0, margin - |mu_m - mu_m'|)^2
 *     L = w_intra L_intra + w_inter L_inter;  M == 0: L = 0 and a zero gradient;  M == 1: L_inter = 0;  a pair whose means are
 *     equal adds margin^2 and no gradient.
 * Outputs, on the device: loss, intra (L_intra), inter (L_inter) fp32 scalars; grad [S,H,W] fp32 = dL/dfeat (0 for an ignored
 * pixel), or NULL: then no gradient is stored; count [K] int64 = n_m; qsum [K,S] int64 = sum over the mask's pixels of
 * rint(f * 2^q) (float64, ties to even) -- exact and free of any order; qexp int32 = q = 40 - e, e the smallest integer with
 * max|f| < 2^e over the WHOLE map (0 for an all-zero map); status int32, 0 or bit 0.  max_abs < 0: the maximum is found by a pass
 * over feat.  max_abs >= 0: e is the smallest integer with max_abs < 2^e and that pass is skipped; a pixel with |f| >= 2^e then
 * counts as +-2^40 and raises bit 0 of status.  Means, pair terms and the residual are float64 in a fixed order; no float
 * atomics, the same bits on every call.  Non-finite features are the caller's error (the call terminates, the numbers mean
 * nothing).  count and qsum may be NULL when K == 0.
 * Refused before any device call: S outside 1..32, H or W < 1, H * W > 2^22, K outside 0..65536 (the workspace size is then 0), a
 * balance other than 0 or 1, a margin that is negative or not finite, a weight that is not finite, a max_abs that is not finite, a
 * NULL required pointer, a pointer that is not 4-byte (count, qsum: 8-byte) aligned, a NULL or misaligned workspace
 * (goi_mask_contrast_workspace_bytes bytes, 256-byte aligned).  Asynchronous on `stream`; returns 0 (or -1: goi_raster_last_error). */
size_t goi_mask_contrast_workspace_bytes(int S, int H, int W, int K);
int goi_mask_contrast(int S, int H, int W, int K, const float* feat, const int32_t* labels, float margin, float w_intra, float w_inter,
                      int balance, float max_abs, float* loss, float* intra, float* inter, float* grad /*[S,H,W] or NULL*/,
                      int64_t* count /*[K]*/, int64_t* qsum /*[K,S]*/, int32_t* qexp, int32_t* status, void* workspace, void* stream);

/* ---- training losses of the semantic head, row pass (train.py:142-163; see csrc/codebook_loss.hip).
 * Inputs: sim_raw [HW][C] = <g_p, LUT_c/|LUT_c|> with g NOT normalised, inv_gnorm [HW] = 1/|g_p|,
 * sem [S][HW] (the rasterizer's channel-major feature map), decoder W [C][S] and bias [C] (or NULL),
 * anneal factor t (1 or 2).  Outputs: dsim [HW][C] = dL/dsim_raw, dsem [S][HW] = dL/dsem, and
 * partials [goi_codebook_loss_partial_rows()][C*(S+1)+4]: per persistent wave the dL/dW rows (S
 * values then dL/db per code) followed by the sums over its pixels of (sum_c (P-label)^2, max sim,
 * entropy, sim at the decoder's argmax); the caller adds the rows up.  L = lab + sl + 0.3 sl1 + recc
 * with upstream gradient 1.  1 <= S <= 16, 1 <= C <= 512.  All pointers are device pointers. */
int goi_codebook_loss_partial_rows(void);
int goi_codebook_loss_rows(const float* sim_raw, const float* inv_gnorm, const float* sem, const float* W,
                           const float* bias, long long HW, int C, int S, float t, float* dsim, float* dsem,
                           float* partials, void* stream);

/* sim_raw [HW][C] = g^T * L1^T and inv_gnorm [HW] = 1/|g_p| in one pass over g [D][HW] (the channel-major ground-truth
 * map), L1 [C][D] the row-normalised code book: the dense code-book x feature contraction of train.py:147-149 on the bf16
 * matrix rate with split (hi + lo) operands, fp32 accumulation (csrc/codebook_loss.hip: codebook_sim_k; products to 2^-16,
 * sim to ~1e-6).  workspace: goi_codebook_sim_workspace_bytes() device bytes.  Supported shape: D = 256, C <= 304, C % 4 = 0;
 * returns < 0 otherwise (use a library GEMM then). */
size_t goi_codebook_sim_workspace_bytes(void);
int goi_codebook_sim(const float* g, const float* lut1, long long HW, int C, int D, float* sim, float* inv_gnorm,
                     void* workspace, void* stream);

/* dL/dL1 [C][D] = dsim^T * g^T as a split-K fp32 MFMA GEMM over the pixel axis (csrc/codebook_loss.hip):
 * dsim [HW][C] (from goi_codebook_loss_rows), g [D][HW] (the channel-major ground-truth map).  Writes
 * partial [goi_codebook_dlut_partial_blocks()][304][D]; the caller sums over the first axis and keeps
 * rows < C.  Supported shape: D = 256, 288 < C <= 304, HW % 4 = 0; returns < 0 otherwise (use a
 * library GEMM then). */
int goi_codebook_dlut_partial_blocks(void);
int goi_codebook_dlut(const float* dsim, const float* g, long long HW, int C, int D, float* partial, void* stream);

/* The three steps above as one call with no [HW][C] fp32 matrix in memory (csrc/codebook_loss.hip: decoder_stats_k,
 * codebook_simgrad_k, decoder_gd_k, codebook_dlut2_k): g [D][HW], lut1 [C][D] (rows normalised), sem [S][HW], W [C][S], bias [C] or NULL, t as in
 * goi_codebook_loss_rows.  Writes dsem [S][HW], partials [goi_codebook_fused_partial_rows()][C*(S+1)+4] (same row format
 * as goi_codebook_loss_rows) and dlut_partial [goi_codebook_dlut_partial_blocks()][304][D]; the caller sums both over the
 * first axis.  workspace: goi_codebook_fused_workspace_bytes(HW) device bytes, 256-byte aligned (dL/dsim as two bf16 planes: 4 bytes per
 * (pixel, code), plus 64 B of records per pixel).  Supported shape: D = 256, 288 < C <= 304, 1 <= S <= 16, HW % 4 = 0,
 * HW < 2^25; anything else returns -1 and the caller uses the three separate entry points.  Reference: train.py:142-163. */
size_t goi_codebook_fused_workspace_bytes(long long HW);
int goi_codebook_fused_partial_rows(void);
int goi_codebook_fused(const float* g, const float* lut1, const float* sem, const float* W, const float* bias, long long HW,
                       int C, int D, int S, float t, float* dsem, float* partials, float* dlut_partial, void* workspace,
                       void* stream);

/* ---- fused Adam step over the Gaussian parameter groups (scene/gaussian_model.py:163-253:
 * torch.optim.Adam(lr=0.0, eps=1e-15) over xyz / f_dc / f_rest / semantics / opacity / scaling /
 * rotation; train.py:193 optimizer.step()) with the optional per-Gaussian gradient mask of
 * gui/main.py:480-513 (clear_noralative_gs_grad: rows with mask != 0 see a zero gradient).
 * One launch for up to GOI_ADAM_MAX_GROUPS tensors.  All pointers are device pointers to fp32,
 * 16-byte aligned; numel = P * row_len. */
#define GOI_ADAM_MAX_GROUPS 8
typedef struct GoiAdamGroup {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    long long numel;
    int row_len;      /* elements per Gaussian (mask granularity); >= 1 */
    float step_size;  /* lr / (1 - beta1^t), rounded to fp32 once */
    float bc2_sqrt;   /* sqrt(1 - beta2^t) */
} GoiAdamGroup;
int goi_adam_step(const GoiAdamGroup* groups, int n_groups, double beta1, double beta2, double eps,
                  const unsigned char* nograd_mask /*[P] or NULL*/, void* stream);
/* The same with a device-side guard: if *skip_flag (a device word, e.g. goi_raster_truncated_flag of the view the
 * gradients came from) is non-zero when the kernel runs, nothing is updated -- parameters and both moments keep their
 * values (the host-side step count of the caller is the caller's business).  skip_flag == NULL: goi_adam_step. */
int goi_adam_step_guarded(const GoiAdamGroup* groups, int n_groups, double beta1, double beta2, double eps,
                          const unsigned char* nograd_mask /*[P] or NULL*/, const uint32_t* skip_flag, void* stream);

/* ---- densification and pruning of the Gaussian set (scene/gaussian_model.py:291-513; csrc/densify.hip).  P < 2^30.
 * All pointers are device pointers to contiguous fp32 rows unless stated; everything is asynchronous on `stream`.
 * goi_raster_densify_stats: add_densification_stats, for every i with filter[i] != 0: accum[i] += sqrt(gx^2 + gy^2),
 *   denom[i] += 1, (gx, gy) = grad[i * grad_stride + 0 / 1] (the 2-D mean gradient, grad_stride >= 2 floats).
 * goi_raster_densify_plan: the decisions of densify_and_prune for every ORIGINAL Gaussian from accum [P], denom [P],
 *   scaling [P][3] (raw log-scales), opacity [P] (raw), each threshold as the reference forms it in double (max_grad,
 *   scale_threshold = percent_dense * extent, min_opacity, big_threshold = 0.1 * extent) and rounded to fp32 here;
 *   screen_test != 0 when max_screen_size is truthy (the reference compares max_screen_size with the ZEROED max_radii2D
 *   then: 0 > max_screen_size prunes every row).  Writes counts (device, 4 words) = rows kept of {originals, clones, first
 *   children, and -- the fourth -- Gaussians selected for a split} and fills the workspace for goi_raster_densify_apply.
 * goi_raster_densify_prune_plan: prune_points: counts[0] = rows with mask[i] == 0 (mask: P bytes), counts[1..3] = 0.
 * goi_raster_densify_apply: after a plan on the same workspace and P: every group reads `rows` = P source rows of row_len
 *   floats and writes the new layout [originals kept][clones kept][first children kept][second children kept] (each block
 *   in ascending original index; dst holds counts[0] + counts[1] + 2 counts[2] rows).  GOI_DENSIFY_PARAM copies a row to
 *   each destination, _MOMENT copies kept originals and writes 0 for clones and children, _XYZ / _SCALING (row_len 3)
 *   form the children's xyz = build_rotation(rotation) @ (Z exp(scaling)) + xyz and scaling = log(exp(s) / 1.6) from
 *   rotation [P][4], scaling [P][3] and z [2 n_split][3] (row r: first child of the split Gaussian of rank r, row n_split + r:
 *   its second child); _ZERO writes `rows` x row_len zeros to dst (src unused).  n_split = counts[3], kept_children =
 *   counts[2].  Up to GOI_DENSIFY_MAX_GROUPS groups in one launch.  No float atomics: the result is deterministic.
 * workspace: goi_raster_densify_workspace_bytes(P) bytes, 256-byte aligned (0: P out of range). */
#define GOI_DENSIFY_MAX_GROUPS 24
#define GOI_DENSIFY_PARAM 0
#define GOI_DENSIFY_MOMENT 1
#define GOI_DENSIFY_XYZ 2
#define GOI_DENSIFY_SCALING 3
#define GOI_DENSIFY_ZERO 4
typedef struct GoiDensifyRows {
    const float* src;
    float* dst;
    long long rows;
    int row_len; /* >= 1 */
    int mode;    /* GOI_DENSIFY_* */
} GoiDensifyRows;
size_t goi_raster_densify_workspace_bytes(long long P);
int goi_raster_densify_stats(long long P, const float* grad, long long grad_stride, const unsigned char* filter, float* accum,
                             float* denom, void* stream);
int goi_raster_densify_plan(long long P, const float* accum, const float* denom, const float* scaling, const float* opacity,
                            double max_grad, double scale_threshold, double min_opacity, int screen_test, double max_screen_size,
                            double big_threshold, unsigned* counts, void* workspace, void* stream);
int goi_raster_densify_prune_plan(long long P, const unsigned char* mask, unsigned* counts, void* workspace, void* stream);
int goi_raster_densify_apply(long long P, const GoiDensifyRows* groups, int n_groups, const float* rotation, const float* scaling,
                             const float* z, long long n_split, long long kept_children, const void* workspace, void* stream);

/* ---- Fixed-budget densification: MCMC relocation and position noise in place (csrc/mcmc.hip) --------------
 * "3D Gaussian Splatting as Markov Chain Monte Carlo" (Kheradmand et al., 2024).  P never changes; everything is a device pointer
 * and asynchronous on `stream`; nothing is read back.  0 <= P < 2^30.
 *
 * goi_mcmc_relocate.  opacity [P] fp32 ACTIVATED (sigmoid of the raw one), read only; draws [n_draws] int64 in [0, 2^32), read
 *   only; selection [P] bytes or NULL (every row): a row with 0 is FROZEN -- never dead, never a source, never written.
 *     dead_i    selected and (double)opacity_i <= min_opacity;  alive_i: selected and (double)opacity_i > min_opacity (a NaN
 *               opacity is neither);  d_0 < d_1 < ... the dead rows in ascending id
 *     w_i       (uint32)(min(opacity_i, 1) * 2^24) for alive rows (exact), 0 otherwise;  C_i = w_0 + ... + w_i (uint64), T = C_{P-1}
 *     moves     min(n_dead, n_draws, max_moves, floor(n_alive * frac_num / frac_den)), in integers on the device; 0 when T == 0
 *     t_j       floor(u_j * T / 2^32) for j < moves, u_j = draws[j] (the high half of the 64 x 64-bit product (u_j << 32) * T)
 *     s_j       min{ i : C_i > t_j } (binary search, at most 32 steps);  r_i = #{ j < moves : s_j = i };  N_i = min(r_i + 1, n_max)
 *   For every source (r_i >= 1), float64 with one rounding to fp32 at the store:
 *     o  = min((double)opacity_i, 1 - 2^-24);   o' = 1 - pow(1 - o, 1 / N)   (N == 1: o' = o)
 *     D  = sum_{m=1..N} sum_{k=0..m-1} (-1)^k (C(m-1, k) * Q[k]) * o'^(k+1): one accumulator in exactly this order, o'^(k+1) a
 *          running product restarted at 1 for each m, odd k subtracted, Q[k] = 1 / sqrt((double)(k + 1)), C(n, k) exact in float64
 *     c  = o / D;   new raw opacity = log(x / (1 - x)), x = min(max(o', min_opacity), 1 - 2^-24);   new raw log-scale = old + log(c)
 *   Written, through the row groups (each `data` holds P rows of row_len floats, in place): dead row d_j receives row s_j of every
 *   GOI_MCMC_PARAM group, and the new opacity / log-scale of s_j in the GOI_MCMC_OPACITY (row_len 1) / GOI_MCMC_SCALING (row_len 3)
 *   group; source i receives the same new opacity and log-scale; every GOI_MCMC_MOMENT row of a SOURCE is zeroed, the dead rows'
 *   moments stay as they were.  Every copy and the source itself see the source's OLD values: the new ones are staged in the
 *   workspace by one kernel and written by a later one.  Nothing else is touched.
 *   Outputs: counts [4] = {moves, n_dead, n_alive, sources hit}; status [1] int32, GOI_MCMC_STATUS_* bits, 0 after a good call;
 *   hits [P] uint32 = r_i, or NULL (they stay in the workspace).  Integer atomics only: the same bits on every call.
 *   P = 0 returns 0 and touches nothing.
 *   Refused before any device call: P or n_draws outside [0, 2^30), max_moves < 0, frac_num outside [0, 2^32], frac_den outside
 *   [1, 2^32], n_max outside 1..51, min_opacity outside [0, 1) (a NaN included), more than GOI_MCMC_MAX_GROUPS groups, a group with
 *   row_len outside [1, 2^20], an unknown mode, a NULL or misaligned pointer, a second opacity or log-scale group or one of another
 *   row length; then, with P > 0: a NULL required pointer, a misaligned one, a NULL or misaligned workspace
 *   (goi_mcmc_relocate_workspace_bytes(P) bytes, 256-byte aligned; 0: P out of range).
 *
 * goi_mcmc_noise: xyz_i += Sigma_i (z_i g_i step) for every selected row, in place, one launch, no workspace.  Float64 throughout,
 *   one rounding at the store: R from the raw quaternion rotation [P,4] normalised as build_rotation does it, s = exp(scaling [P,3]),
 *   Sigma = (R diag s)(R diag s)^T, g = 1 / (1 + exp(-k ((1 - opacity) - x0))) with opacity [P] ACTIVATED, z [P,3] the caller's normal
 *   draws, step = noise_lr * lr_xyz.  A frozen row (selection 0) is not written.  Refused: P out of range, a k, x0 or step that is
 *   not finite, a NULL or misaligned pointer.
 *
 * goi_mcmc_debug_relocation_sum: D[i] for o_new[i] (float64) and N[i] (clamped to 1..51), n <= 2^24: the device function the
 *   relocation uses, for a test that holds the sum to its restatement bit for bit. */
#define GOI_MCMC_MAX_GROUPS 24
#define GOI_MCMC_PARAM 0   /* a plain parameter: dead rows receive their source's row */
#define GOI_MCMC_OPACITY 1 /* the raw opacity (row_len 1) */
#define GOI_MCMC_SCALING 2 /* the raw log-scale (row_len 3) */
#define GOI_MCMC_MOMENT 3  /* an Adam moment: the sources' rows are zeroed */
#define GOI_MCMC_STATUS_DRAW 1   /* a draw outside [0, 2^32): its low 32 bits were used */
#define GOI_MCMC_STATUS_SEARCH 2 /* a search ran out of its bound (cannot happen: t_j < T = C_{P-1}) */
typedef struct GoiMcmcRows {
    float* data;
    int row_len;
    int mode; /* GOI_MCMC_* */
} GoiMcmcRows;
size_t goi_mcmc_relocate_workspace_bytes(long long P);
int goi_mcmc_relocate(long long P, const float* opacity, const int64_t* draws, long long n_draws, const unsigned char* selection,
                      double min_opacity, long long max_moves, long long frac_num, long long frac_den, int n_max,
                      const GoiMcmcRows* groups, int n_groups, unsigned* hits /*[P] or NULL*/, unsigned* counts /*[4]*/,
                      int32_t* status, void* workspace, void* stream);
int goi_mcmc_noise(long long P, float* xyz, const float* rotation, const float* scaling, const float* opacity, const float* z,
                   const unsigned char* selection, double k, double x0, double step, void* stream);
int goi_mcmc_debug_relocation_sum(int n, const double* o_new, const int32_t* N, double* D, void* stream);

/* ---- Non-rigid edits: as-rigid-as-possible deformation of a selection (csrc/deform.hip) --------------------
 * Control nodes with rest positions x [M,3] on a graph idx [M,k] int32 (what goi_knn_graph returns), optional weight [M,k] (NULL: 1),
 * and the graph's transpose in_ptr [M+1] / in_edge [M*k] (goi_knn_transpose).  Entry (i, m) is an edge iff 0 <= idx[i,m] < M and
 * idx[i,m] != i; anything else is skipped and never used as an address.  Everything is a device pointer and asynchronous on `stream`;
 * nothing is read back; no float atomics: the same bits on every call.  M * k < 2^30.
 *
 *     E = sum_i sum_{edges (i, m), j = idx[i,m]} w[i,m] |(y_i - y_j) - R(q_i) (x_i - x_j)|^2
 *
 * goi_deform_solve: y [M,3] and q [M,4] (w, x, y, z) hold the warm start on entry and the result on return.  `iterations` times:
 *   POSITIONS (Jacobi, from the old y and q): a node with constrained[i] != 0 takes target[i]; a free node with
 *   W = sum_out w + sum_in w > 0 takes (1 - relax) y_i + relax yhat_i, computed as y_i + relax (yhat_i - y_i) with
 *   yhat_i - y_i = [sum_out w ((y_j - y_i) + R_i (x_i - x_j)) + sum_in w ((y_m - y_i) - R_m (x_m - x_i))] / W, out-edges in row order,
 *   then in-edges in in_edge order, one accumulator (an undeformed graph gives exact zeros and keeps y's bits); W <= 0 keeps y_i.
 *   Then ROTATIONS: A_i = sum_out w ((y_i - y_j)(x_i - x_j)^T) (symmetric bit for bit when y = x: no torque) and polar_iters
 *   steps of omega = (sum_c r_c x a_c) / (|sum_c r_c . a_c| + 1e-9), q <- normalize(exp(omega) (x) q) over the columns r_c of R(q),
 *   a_c of A_i; a zero omega, or one whose length is not finite, leaves q bit for bit.  constrained NULL: no node is constrained.  iterations = 0 or M = 0 returns 0 and
 *   touches nothing.  Refused: M < 0, k < 1, M * k >= 2^30, iterations < 0, polar_iters < 0, relax outside (0, 1] (a NaN included);
 *   then a NULL required pointer, a misaligned one, a NULL or misaligned workspace (goi_deform_solve_workspace_bytes(M) bytes).
 *
 * goi_deform_energy: *energy (float64, device) = E, every term formed in float64 and summed in a fixed order.
 *
 * goi_deform_apply: one launch over the P Gaussians.  A row takes part iff it is selected (selection [P] bytes, NULL: every row;
 *   invert: the rows whose byte is 0) and its binding row bind_idx [P,kb] / bind_dist2 [P,kb] (the rows goi_knn_graph writes for the Gaussians as queries
 *   and the nodes as references: knn.query) has a USED entry: 0 <= id < n_nodes and a finite distance.  With d_0^2 the first used entry's distance,
 *   w_a = exp(-(d_a^2 - d_0^2) * (1 / (2 sigma^2))) normalised by their sum in entry order.  moments = 0 (source: the REST tensors
 *   src_*, destination: the model, which may be the same memory):
 *     xyz      = x + sum_a w_a [(y_a - x_a) + (R(q_a) - I)(x - x_a)]   (R - I from the quaternion's terms; a zero sum keeps x's bits)
 *     q_g      = normalize(sum_a w_a s_a q_a), s_a = -1 where q_a . q_first < 0;  rotation = q_g (x) src_rotation
 *     features_rest [P, M - 1, 3]: every stored band l = 1..3 times D_l(R(q_g)) per channel, built per row as
 *              D_l c = inv_l (Y_l(R^T dirs_l) c) from the constants of GoiDeformSH
 *     a row whose q_g has a zero vector part gets src_rotation's and src_features_rest's bits.
 *   moments = 1 (in place; src_* are not read; any of xyz, rotation, features_rest may be NULL): the rows' Adam first moments
 *     turned by the same q_g: xyz <- R(q_g) m, rotation <- q_g (x) m, features_rest <- D_l m; a row with the identity is not written.
 *   Rows that do not take part are neither read nor written.  P = 0 or n_nodes = 0 returns 0 and touches nothing.
 *   Refused: P outside [0, 2^31), M not in 1, 4, 9, 16, n_nodes outside [0, 2^30), kb outside 1..8, P * kb >= 2^31, a sigma that is
 *   not finite and > 0, moments not 0 or 1, sh NULL; then a NULL required pointer or a misaligned one. */
typedef struct GoiDeformSH {
    float dirs1[9], dirs2[15], dirs3[21]; /* 2 l + 1 unit directions per band, [n][3] */
    float inv1[9], inv2[25], inv3[49];    /* the inverse of the band's basis at those directions, row-major */
} GoiDeformSH;
size_t goi_deform_solve_workspace_bytes(int M);
int goi_deform_solve(int M, int k, const float* x, const int32_t* idx, const float* weight, const int32_t* in_ptr,
                     const int32_t* in_edge, const unsigned char* constrained, const float* target, int iterations, int polar_iters,
                     float relax, float* y, float* q, void* workspace, void* stream);
size_t goi_deform_energy_workspace_bytes(int M);
int goi_deform_energy(int M, int k, const float* x, const int32_t* idx, const float* weight, const float* y, const float* q,
                      double* energy, void* workspace, void* stream);
int goi_deform_apply(long long P, int M, int n_nodes, int kb, const unsigned char* selection, int invert, const int32_t* bind_idx,
                     const float* bind_dist2, float sigma, const float* node_x, const float* node_y, const float* node_q,
                     const GoiDeformSH* sh, const float* src_xyz, const float* src_rotation, const float* src_features_rest,
                     float* xyz, float* rotation, float* features_rest, int moments, void* stream);

/* Lane utilisation of the blend kernels, counted on the device from what the forward of a frame left in its workspaces
 * (member masks, n_contrib, per-quadrant walk lengths): a diagnostic of the execution mapping, not part of the reference's
 * interface (its blend loops, one thread per pixel: CR/forward.cu:330-372, CR/backward.cu:523-589).  R / the three buffers:
 * as for goi_raster_backward of the same frame.  counters: DEVICE array of GOI_BLEND_STATS_WORDS 64-bit words, cleared
 * and filled on `stream`:
 *   0 quadrants (8x8 pixels = one wave) that composited anything      1 rounds of 64 list positions they walk
 *   2 list positions in those rounds up to the quadrant's last contributor
 *   3 of those, candidates passing the forward's quadrant hit test (the pairs the forward blend evaluates)
 *   4 MEMBER pairs: (quadrant, Gaussian) with a contribution to some pixel (the pairs the backward evaluates and flushes)
 *   5 live lanes: (pixel, Gaussian) contributions = lanes doing useful work, summed over the member pairs
 *   6 / 7 / 8 (block, Gaussian) pairs with a live lane were a wave split into 8x4 / 4x4 / 2x2 pixel blocks
 *   9 member pairs without a live lane (0 by construction)   10 pixels inside the image   11 sum of n_contrib */
#define GOI_BLEND_STATS_WORDS 16
int goi_raster_blend_stats(int P, int W, int H, int R, const void* geom_buffer, const void* binning_buffer,
                           const void* image_buffer, unsigned long long* counters, void* stream);

/* Peak blend weight per Gaussian and the dominant contributor per pixel of a finished frame: one replay of its tile lists with
 * the forward's own pair evaluation (candidates by the quadrant hit test; a pixel is live until a pair that passes both alpha
 * guards fails T (1 - alpha) >= 1e-4), no feature arithmetic.  Not part of the reference's interface.  R / the three buffers:
 * as for goi_raster_backward of the same frame.  DEVICE outputs, written on `stream`; each may be NULL, not all three:
 *   peak   [P] float32: merged BY MAXIMUM with what is there (zero it once, sweep any number of views): the largest
 *          w = alpha * T of the Gaussian over every live pixel inside the image -- over its contributions and over the pair that
 *          ended a pixel, whose w is what the Gaussian would have added.  peak == 0 over a set of frames: the Gaussian never
 *          passed the guards on a live pixel of any of them; removing it changes no output map of those frames in any bit.
 *          Merged with an integer atomic maximum on the bit patterns (w >= 0): the same bits whatever the order.
 *   top_id [H*W] int32, top_w [H*W] float32: the pixel's contributor of largest w (the front-most of equals; the pair that
 *          ended the pixel added nothing and is not one) and that w; -1 and 0 where nothing contributed.
 * A truncated frame (goi_raster_truncated_flag) merges nothing into peak and writes -1 / 0; so does R == 0, without a launch. */
int goi_raster_contrib_frame(int P, int W, int H, int R, const void* geom_buffer, const void* binning_buffer,
                             const void* image_buffer, float* peak, int* top_id, float* top_w, void* stream);

/* Lifts a 2D label map onto the Gaussians by exact blend-weight votes: the same replay as goi_raster_contrib_frame, and for
 * every pair that CONTRIBUTES to a pixel inside the image (both guards passed on a live pixel and T (1 - alpha) >= 1e-4; the
 * pair that ended a pixel added nothing to the picture and is excluded, which also makes the sums those of the backward with a
 * one-hot upstream) with l = labels[pixel] in [0, K):
 *     votes[id * K + l] += q,   q = w * 2^24 rounded half-to-even to an integer,  w = alpha * T
 * (the product is exact in fp32; w >= 1e-4 / 255 > 2^-25, so q >= 1: a Gaussian's total is non-zero exactly when it contributed
 * to a validly labelled pixel).  One vote unit is 2^-24 of a pixel's full weight.
 *   labels [H*W] int32, DEVICE: any value outside [0, K) (negative, K, INT_MAX ...) is ignored -- the "don't know" band.
 *   votes  [P*K] int64, DEVICE: ADDED TO on `stream` (zero it once, sweep any number of views and label maps).  Integer sums
 *          by 64-bit integer atomics, one per (8x8 quadrant, Gaussian, label) after a wave sum: the same bits in any order.
 * R / the three buffers: as for goi_raster_contrib_frame.  A truncated frame adds nothing; so does R == 0, without a launch. */
int goi_raster_contrib_votes(int P, int W, int H, int R, const void* geom_buffer, const void* binning_buffer,
                             const void* image_buffer, const int* labels /*[H*W]*/, int K,
                             int64_t* votes /*[P*K], added to*/, void* stream);

/* Inspection of the opaque workspaces (tests only): copies device -> caller DEVICE buffers.
 * Any pointer may be NULL.  point_list is in final sorted order. */
int goi_raster_debug_views(int P, int W, int H, int R, const void* geom_buffer, const void* binning_buffer,
                           const void* image_buffer,
                           float* depths /*[P]*/, float* means2D /*[P,2]*/, float* conic_opacity /*[P,4]*/,
                           float* rgb /*[P,3]*/, uint32_t* tiles_touched /*[P]*/, uint32_t* point_list /*[R]*/,
                           uint32_t* ranges /*[T,2]*/, uint32_t* n_contrib /*[H*W]*/, void* stream);

/* The device-wide radix sort and scan every stage sorts and scans with (tests only).  Both follow the option snapshot
 * (goi_raster_set_option "sort_variant" / "sort_small" / "sort_lookback") and are asynchronous on `stream`.
 * Sort: stable ascending sort of (keys0, vals0) on key bits [lo, hi), 0 <= lo < hi <= 32, n < 2^30; keys1 / vals1 are the
 * ping-pong buffers.  Returns the index (0/1) of the buffers that hold the result, or < 0 (goi_raster_last_error).
 *   n_dev    (device, may be NULL): the count; n is then a capacity and min(*n_dev, n) keys are sorted.  Onesweep only.
 *   ghist    (device, may be NULL): [passes][256] digit histograms of the keys sorted, passes = ceil((hi - lo) / 8) over
 *            [lo, hi) split as evenly as possible, low digits first.  The sort's histogram kernel is then skipped.  Onesweep only.
 *   flags    bit 0: the caller has zeroed the workspace's control words (the whole workspace will do).
 *   error_out (device, may be NULL): gets the sort's error bits OR-ed in (non-zero: the result is not to be used).
 *   workspace: goi_raster_debug_sort_workspace_bytes(n, lo, hi) bytes, 256-byte aligned.
 * Scan: out[i] = sum of f(j) over j < i, f(j) = gather ? in[gather[j]] : in[j], mod 2^32; *total (device, may be NULL) =
 * the sum.  n_dev as above (out[count .. n) is not written).  out == in is allowed only without a gather.
 *   workspace: goi_raster_debug_scan_workspace_bytes(n) bytes. */
size_t goi_raster_debug_sort_workspace_bytes(long long n, int lo, int hi);
int goi_raster_debug_sort_pairs(uint32_t* keys0, uint32_t* vals0, uint32_t* keys1, uint32_t* vals1, long long n, int lo, int hi,
                                const uint32_t* n_dev, const uint32_t* ghist, int flags, uint32_t* error_out, void* workspace,
                                void* stream);
size_t goi_raster_debug_scan_workspace_bytes(long long n);
int goi_raster_debug_exclusive_scan(const uint32_t* in, const uint32_t* gather, uint32_t* out, long long n, const uint32_t* n_dev,
                                    uint32_t* total, void* workspace, void* stream);

/* The backward's row reduction (tests only): sums the partial-gradient rows of a frame with the product's launchers, on caller
 * buffers, asynchronously on `stream`.  Slot = (emit-order instance) * 4 + quadrant; rows [4 n_cap][row_floats], validity bytes
 * flags [4 n_cap] (non-zero: the row is added).  The listed Gaussian of depth rank i (i < V <= P) is order[i] and owns the
 * instances [offsets[i], offsets[i + 1]) -- the last one up to the count --, clamped to min(count, n_cap); a frame whose overflow
 * word is non-zero owns none.  A Gaussian's rows are added in 16-instance chunks counted from its first instance, inside a
 * chunk quadrant-major (all quadrant-0 rows of the chunk's instances, then quadrant 1, ...).
 *   mode 0: the six per-id arrays of goi_raster_backward (bwd_records 0), every element of all P Gaussians written
 *   mode 1: one record per listed Gaussian that owns an instance, over its first slot's row (bwd_records 1)
 *   mode 2: records of the big Gaussians only (bwd_records 2; 128-byte rows, S = 5 .. 20)
 *   mode 3: dL_dsemantic of the semantics-only backward (rows of the padded semantic channels only)
 * frame (device): {count, listed V, overflow}.  tiles_touched [P] (non-zero: listed) is read by modes 0 and 3, the arrays by
 * modes 0 (all six) and 3 (dL_dsemantic); the other pointers may be NULL there.
 * goi_raster_debug_reduce_row_floats: the row width the mode lays out for S, or < 0 (goi_raster_last_error).
 * workspace: goi_raster_debug_reduce_workspace_bytes(n_cap) bytes, 256-byte aligned: a 256-byte counter block, then the
 * 8 control words of the big Gaussians (at byte 256; word 1: huge ones registered, word 2: the other big ones), then their
 * descriptors. */
int goi_raster_debug_reduce_row_floats(int mode, int S);
size_t goi_raster_debug_reduce_workspace_bytes(long long n_cap);
int goi_raster_debug_reduce_rows(int mode, int P, int S, long long n_cap, const uint32_t* frame, const uint32_t* order,
                                 const uint32_t* offsets, const uint32_t* tiles_touched, float* rows, const uint8_t* flags,
                                 float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dsemantic,
                                 float* dL_ddepth, void* workspace, void* stream);

/* The per-Gaussian backward (tests only): the product's own launch of preprocess_bwd_k on caller buffers, asynchronously on
 * `stream`; nothing comes from a forward pass.  From `scene`: P, D, M, S, W, H, means3D, shs (or NULL: no SH path), scales +
 * rotations (or NULL: no scale / rotation path; cov3D_precomp is then the covariance), scale_modifier, the camera.  All arrays
 * are DEVICE arrays:
 *   radii [P] (> 0: visible -- the caller's choice), clamped [P] (bit 0..2: r, g, b clamped; read with shs only), cov3D [P,6]
 *   (what the forward computed from scale / rotation; unused with cov3D_precomp), prev_radii [P] or NULL (the radii of the
 *   backward that last wrote these output buffers: a Gaussian invisible then and now is left untouched),
 *   frame {count, listed, overflow}: copied into the counter block at the start of `workspace` (256 bytes, 256-byte aligned);
 *   a non-zero overflow word makes every Gaussian invisible.
 * source: where the blend gradients of a Gaussian come from
 *   0  the per-id arrays dL_dmean2D [P,3], dL_dconic [P,4] (a, b, -, c), dL_dcolor [P,3], dL_ddepth [P] (inputs; dL_dcolor is
 *      rewritten in factored mode);
 *   1  its RECORD in `rows` over the slot 4 * aux[4 g] (aux [P,4] words, word 0: first emit-order instance) when
 *      tiles_touched[g] != 0, zeros otherwise; the kernel writes dL_dmean2D, dL_dcolor, dL_dopacity [P], dL_dsemantic [P,S];
 *      record = [sem 0 .. 4 ceil(S/4)) | r g b depth | mean2D x y | conic a b c | opacity], row width as
 *      goi_raster_debug_reduce_row_floats(1, S);
 *   2  the kernel sums the rows of the Gaussian's tiles_touched[g] instances from aux[4 g] on (validity bytes row_flags
 *      [4 n_cap], order as goi_raster_debug_reduce_rows), or reads its record when it has more instances than the frame's
 *      big-Gaussian threshold; 128-byte rows only.  Every instance must lie below n_cap.
 * flags: GOI_BACKWARD_ACCUMULATE (source 1, prev_radii NULL, dL_dsh given with shs): visible rows are added to, the others kept.
 * dL_dsh NULL with shs: factored mode (the clamp-masked colour gradient goes to dL_dcolor).  max_blocks > 0 caps the persistent
 * grid (0: the product's choice).  Outputs: dL_dmean3D [P,3], dL_dcov3D [P,6], dL_dsh [P,M,3], dL_dscale [P,3], dL_drot [P,4].
 * Invalid combinations fail by name (goi_raster_last_error). */
int goi_raster_debug_preprocess_backward(const GoiRasterScene* scene, int source, int flags, int max_blocks, long long n_cap,
                                         const uint32_t* frame, const int* radii, const uint8_t* clamped, const float* cov3D,
                                         const int* prev_radii, const uint32_t* aux, const uint32_t* tiles_touched,
                                         const float* rows, const uint8_t* row_flags, float* dL_dmean2D, const float* dL_dconic,
                                         float* dL_dopacity, float* dL_dcolor, float* dL_dsemantic, const float* dL_ddepth,
                                         float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                                         void* workspace, void* stream);

/* One (pixel, Gaussian) evaluation of the blend kernels, written out (tests only), asynchronously on `stream`.  Every blend
 * kernel evaluates a pair through the same two device functions (csrc/blend_common.h: poly_coefs, eval_poly); this entry runs
 * them for caller-chosen pairs of a frame whose forward filled geom_buffer (the records are read from it).
 *   requests [n_requests][2] (DEVICE, 8-byte aligned): (Gaussian id, quadrant index 4 * tile + q; q = 0..3: the 8x8 pixel
 *     quadrants of the 16x16 tile in row-major order, tiles row-major as everywhere).  One wave per request, one pixel per lane:
 *     lane l is pixel (l & 7, l >> 3) of the quadrant, whether it lies inside the image or not.
 *   E, alpha [n_requests][64]: opacity * exp(power) before the 0.99 clamp, and alpha = min(0.99, E);
 *   guards [n_requests][64]: bit 0 "below" (the exponent passes the power <= tolerance guard), bit 1 "seen" (alpha >= 1/255); a pair
 *     contributes where both are set.  A request that names no Gaussian (id >= P) or no quadrant gets NaN and 0x80.
 * The records are the FIRST array of the geometry workspace, [P] x 12 floats (x, y, conic a, b | conic c, opacity, hx, hy | r, g, b,
 * depth); only the first six are read here, so a test may also write records of its own into a zeroed workspace.
 * Requests are processed 2^20 per launch. */
int goi_raster_debug_pair_eval(int P, int W, int H, const void* geom_buffer, const uint32_t* requests, long long n_requests,
                               float* E, float* alpha, uint8_t* guards, void* stream);

/* The backward BLEND stage alone, on a real frame (tests only), asynchronously on `stream`: what goi_raster_backward /
 * goi_raster_backward_semantics run before the row reduction -- the quadrant-order launch (or the memsets) and one blend kernel,
 * through the product's launchers -- and copies of what it left.  From `scene`: P, S, W, H, bg, semantics.  R, the three
 * workspaces, radii, out_alpha: as for goi_raster_backward of the same frame (R > 0).  The four upstream gradients may each be
 * NULL (zero).  mode selects the kernel whatever goi_raster_set_option says:
 *   0..3  render_bwd_rows_k: bit 0 set = exact-fp32 flush (else split-f16), bit 1 set = candidate testing (else member masks);
 *   4..7  render_bwd_sem_k (rows of the padded semantic channels only), same two bits; needs dL_dout_semantic;
 *   8     render_bwd_tile_k: the six per-id arrays of goi_raster_backward (zeroed, then accumulated with atomics).
 * Modes 0..7 need `scratch` (goi_raster_backward_scratch_bytes(R, S), 256-byte aligned; rows the kernel does not write keep
 * what the caller left there) and copy out  rows [4 R][row_floats] (row_floats = goi_raster_debug_reduce_row_floats(1, S), or
 * (3, S) for modes 4..7; 16-byte aligned) and row_flags [4 R].  Row layout of modes 0..3:
 *   [sem 0 .. 4 ceil(S/4)) | r g b depth | mean2D x y (NDC units) | conic a b c | opacity | pad]
 * slot = 4 * (emit-order instance) + quadrant; a Gaussian's first instance is word 0 of its aux entry.
 * Every mode copies out, where the pointer is not NULL:  aux [P][4] words;  qmask0 [4 T] and qmask [4 (R / 64 + 2)] 64-bit
 * member words as the forward left them (round 0 of quadrant q of tile t: qmask0[4 t + q]; round r >= 1 of a tile whose list
 * starts at x0: qmask[4 (x0 / 64 + r) + q]; bit j: list position 64 r + j contributed to some pixel of the quadrant);
 * qcost [4 T];  qorder [8 ceil(4 T / 8)] when the quadrant order exists.
 * Returns 1 when the quadrant order was launched (qorder written), 0 when not, < 0 on error (goi_raster_last_error). */
int goi_raster_debug_backward_blend(const GoiRasterScene* scene, int R, int mode, const void* geom_buffer,
                                    const void* binning_buffer, const void* image_buffer, const int* radii,
                                    const float* out_alpha, const float* dL_dout_color, const float* dL_dout_semantic,
                                    const float* dL_dout_depth, const float* dL_dout_alpha, void* scratch, float* rows,
                                    uint8_t* row_flags, uint32_t* aux, unsigned long long* qmask0, unsigned long long* qmask,
                                    uint32_t* qcost, uint32_t* qorder, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity,
                                    float* dL_dcolor, float* dL_dsemantic, float* dL_ddepth, void* stream);

/* ---- a mesh from the Gaussians (csrc/field.hip) ---------------------------------------------------------
 * goi_field_density: DreamGaussian's extract_fields(resolution, num_blocks, relax_ratio), which the reference's viewers
 * presuppose (gui/main.py:607-617 calls extract_mesh; gui/gs_renderer.py:66-85 keeps only gaussian_3d_coeff).  Asynchronous on
 * `stream`, nothing read back, no float atomics: the same bits every run.
 *   kept        opacity[i] > (float)min_opacity, selected (selection NULL: all; otherwise (selection[i] != 0) != selection_invert),
 *               and a finite centre.  The model is read in place.
 *   frame       out, 4 floats: center = (min + max) / 2 of the kept centres, scale = (float)(1.8 / max extent); bounds != NULL
 *               (device, 4 floats: center, scale) replaces it.  Nothing kept: (0, 0, 0, 1); no extent: scale 1.
 *   inputs      xyz [P][3], opacity [P] (activated), scaling [P][3] (activated), rotation [P][4] (raw: normalised here),
 *               attributes [P][3] or NULL.  Centre and scales are multiplied by scale; covariance (R S)(R S)^T as
 *               build_scaling_rotation / strip_symmetric and its inverse by gaussian_3d_coeff's formulas (1 / (det + 1e-24)), in
 *               fp64 once per Gaussian; the weight as gaussian_3d_coeff writes it in fp32 (power > 0: 0).
 *   grid        coords [resolution] = torch.linspace(-1, 1, resolution) (read, never recomputed); block_lo / block_hi [num_blocks]:
 *               the point bounds of block b, coords[b split] and coords[(b + 1) split - 1], widened by (2 / num_blocks) relax_ratio
 *               in fp32; split = resolution / num_blocks.  A Gaussian joins block (bx, by, bz) iff lo < centre < hi strictly on every
 *               axis.  occ [R][R][R] (x, y, z) = sum opacity w over the block's members; attr_out [3][R][R][R] = sum opacity w a
 *               (attributes != NULL).
 *   limits      0 <= P < 2^30, GOI_FIELD_MIN_SPLIT <= split <= GOI_FIELD_MAX_SPLIT, resolution <= GOI_FIELD_MAX_RESOLUTION,
 *               resolution % num_blocks == 0, 0 <= relax_ratio <= GOI_FIELD_MAX_RELAX.  Anything else: -1.
 *   status      out, one word: 0, or bit 1 when the sort's look-back timed out (the grids are then garbage: a caller that reads
 *               anything back must look at it first, as field.extract_mesh does).
 *   workspace   goi_field_density_workspace_bytes(P, resolution, num_blocks, relax_ratio) bytes (0: bad arguments), 256-byte aligned.
 * GOI_FIELD_BATCH: members a block collects in LDS before its threads add them to their points (the sum does not depend on it).
 *
 * goi_field_iso_count / goi_field_iso_emit: marching tetrahedra on the Kuhn split of every cube of a [X][Y][Z] fp32 grid.  A point
 * is inside iff value > (float)thresh.  A grid point owns seven edges (slots +x +y +z +xy +xz +yz +xyz); a vertex exists on an
 * owned edge whose end points differ, at p_a + t (p_b - p_a), t = (thresh - v_a) / (v_b - v_a), a the owner, every operation one
 * fp32 rounding; its colour is (A_a + t (A_b - A_a)) / thresh (attr [3][X][Y][Z] or NULL).  cx / cy / cz: the coordinates of the
 * grid lines per axis, or NULL for the index itself.  Vertices are ordered by (owner, slot), faces by (cube, tetrahedron, triangle),
 * normals point from inside to outside, the surface is open where it meets the grid's boundary.
 *   count: fills the workspace and writes counts[0] = vertices, counts[1] = faces (device): the caller reads them back, sizes
 *          vertices [V][3], faces [F][3] (int32), colors [V][3] and calls emit with the same grid, thresh and workspace.
 *   workspace: goi_field_iso_workspace_bytes(X, Y, Z) bytes (0: bad dimensions), 256-byte aligned.  1 <= X, Y, Z and X Y Z <= GOI_FIELD_MAX_GRID_POINTS = 2^26 (a
 *          point owns at most 7 crossings and a cube has at most 12 triangles, so both counts stay below 2^31 and their sum, which
 *          one 32-bit scan forms, below 2^32). */
#define GOI_FIELD_BATCH 128
#define GOI_FIELD_MIN_SPLIT 4
#define GOI_FIELD_MAX_SPLIT 16
#define GOI_FIELD_MAX_RESOLUTION 256
#define GOI_FIELD_MAX_RELAX 4.0
#define GOI_FIELD_MAX_GRID_POINTS (1ll << 26)
size_t goi_field_density_workspace_bytes(long long P, int resolution, int num_blocks, double relax_ratio);
int goi_field_density(long long P, const float* xyz, const float* opacity, const float* scaling, const float* rotation,
                      const uint8_t* selection, int selection_invert, double min_opacity, const float* attributes,
                      const float* bounds, int resolution, int num_blocks, double relax_ratio, const float* coords,
                      const float* block_lo, const float* block_hi, float* occ, float* attr_out, float* frame, int* status,
                      void* workspace, void* stream);
size_t goi_field_iso_workspace_bytes(int X, int Y, int Z);
int goi_field_iso_count(const float* grid, int X, int Y, int Z, double thresh, void* workspace, int* counts, void* stream);
int goi_field_iso_emit(const float* grid, const float* attr, int X, int Y, int Z, double thresh, const float* cx, const float* cy,
                       const float* cz, const void* workspace, long long n_vertices, long long n_faces, float* vertices, int* faces,
                       float* colors, void* stream);

/* ---- Mesh clean-up (csrc/mesh.hip) -----------------------------------------------------------------------
 * A mesh is vertices [V][3] fp32 and faces [F][3] int32, both on the device; 0 <= V, F and V, 3 F < 2^30.  Every entry point
 * runs on `stream`, returns 0 (or -1: goi_raster_last_error) and never reads the device back; workspaces are the matching
 * *_workspace_bytes(V, F) bytes (0: bad sizes), 256-byte aligned.  Integer outputs are exact, float outputs have one fixed
 * summation order and no float atomics: two calls give the same bits.  All float arithmetic is one fp32 rounding per operation.
 * `status` words are device words holding GOI_MESH_STATUS_* bits: a caller that reads results back looks at them first.
 *
 * goi_mesh_components: two vertices are connected when a face names both.  vertex_label [V] = the smallest vertex index of the
 *   vertex's component, -1 for a vertex no face names; face_label [F] = the label of the face's first vertex.
 * goi_mesh_clean_plan / _emit: in this order, drops null faces (a repeated index, a non-finite vertex, or the cross product
 *   (v1 - v0) x (v2 - v0) exactly zero), duplicate faces (the same set of three indices; the lowest face stays), components
 *   with fewer than min_faces faces or with d2 < min_diag2 * d2 of the mesh (d2: the fp64 sum, x y z, of the squares of the fp32
 *   extents of the box of the vertices still referenced), and unreferenced vertices.  plan writes counts[0] = vertices,
 *   counts[1] = faces, counts[2] = status; the caller reads them back, sizes the outputs and calls emit with the same mesh and
 *   workspace.  Survivors keep their order; vertex_index / face_index give their original indices; colors [V][3] or NULL.
 * goi_mesh_decimate_*: vertex clustering on a divisions^3 grid over the box of the members (finite vertices a face names):
 *   lo = the per-axis minimum, cell = (largest extent) / divisions, q = min(floor((v - lo) / cell), divisions - 1), key =
 *   (qx n + qy) n + qz; no extent: cell 0.  members: once per mesh.  probe: *count = faces whose three vertices are members in
 *   three distinct cells.  plan: sorts, maps the faces through the cells, drops those without three distinct cells and duplicates,
 *   writes counts as clean_plan does and returns (0 or 1) the value emit wants as sorted_in.  emit: vertices (and colours) = the
 *   mean of a cell's members, summed in fp64 in ascending vertex index, divided by the count and rounded once; only cells a
 *   surviving face names, by ascending key; cluster [V] = the output vertex of every input vertex or -1.  1 <= divisions <= 1024.
 * goi_mesh_normals: Mesh.auto_normal -- every face adds its un-normalised cross product to its three corners; here each vertex
 *   sums its corners in ascending (face, corner) order; a sum with dot <= 1e-20 becomes (0, 0, 1); divided by
 *   sqrt(max(dot, 1e-20)). */
#define GOI_MESH_STATUS_SORT 2   /* a look-back of a sort timed out on a wedged device: the results are garbage */
#define GOI_MESH_STATUS_UNION 4  /* a union-find walk ran out of its bound (cannot happen: parents only decrease) */
#define GOI_MESH_STATUS_RANGE 8  /* a face names an index outside [0, V): it was treated as absent */
#define GOI_MESH_MAX_DIVISIONS 1024
size_t goi_mesh_components_workspace_bytes(long long V, long long F);
int goi_mesh_components(long long V, long long F, const int* faces, int* vertex_label, int* face_label, int* status,
                        void* workspace, void* stream);
size_t goi_mesh_clean_workspace_bytes(long long V, long long F);
int goi_mesh_clean_plan(long long V, long long F, const float* vertices, const int* faces, long long min_faces, double min_diag2,
                        void* workspace, int* counts, void* stream);
int goi_mesh_clean_emit(long long V, long long F, const float* vertices, const int* faces, const float* colors,
                        const void* workspace, long long n_vertices, long long n_faces, float* out_vertices, int* out_faces,
                        float* out_colors, int* vertex_index, int* face_index, void* stream);
size_t goi_mesh_decimate_workspace_bytes(long long V, long long F);
int goi_mesh_decimate_members(long long V, long long F, const float* vertices, const int* faces, void* workspace, void* stream);
int goi_mesh_decimate_probe(long long V, long long F, const float* vertices, const int* faces, int divisions, void* workspace,
                            int* count, void* stream);
int goi_mesh_decimate_plan(long long V, long long F, const float* vertices, const int* faces, int divisions, void* workspace,
                           int* counts, void* stream);
int goi_mesh_decimate_emit(long long V, long long F, const float* vertices, const float* colors, int divisions, int sorted_in,
                           const void* workspace, long long n_vertices, long long n_faces, float* out_vertices, int* out_faces,
                           float* out_colors, int* cluster, void* stream);
size_t goi_mesh_normals_workspace_bytes(long long V, long long F);
int goi_mesh_normals(long long V, long long F, const float* vertices, const int* faces, float* normals, int* status,
                     void* workspace, void* stream);

/* ---- Texture bake (csrc/texture.hip) ----------------------------------------------------------------------
 * What gui/main.py:614-752 (save_model, mode 'geo+tex') does with nvdiffrast, grid_put.py, scipy and sklearn.  Every pointer is
 * a device pointer; every entry point runs on `stream`, returns 0 (or -1: goi_raster_last_error) and never reads the device
 * back; workspaces are the matching *_workspace_bytes bytes (0: bad sizes), 256-byte aligned.  No float atomics: two calls
 * give the same bits.  All float arithmetic is one fp32 rounding per operation, in the order DESIGN.md 4.22 writes down.
 * `status` words are device words holding GOI_TEXTURE_STATUS_* bits.
 *
 * goi_texture_rasterize: v_clip [V][4] clip-space positions, faces [F][3].  Screen position = ((x / w + 1) size - 1) / 2 (pixel
 *   centres at integers, the Gaussian rasterizer's mapping), snapped to 1/256 pixel (round half to even); coverage by 64-bit
 *   integer edge functions with a top-left rule; no culling; a face with a w <= 0, a position beyond 2^20 pixels or no area draws
 *   nothing.  Depth = z / w interpolated with the perspective-correct barycentrics; the nearest wins, equal bits go to the lower
 *   face.  tri [H][W] = face + 1 or 0, bary [H][W][2] = the weights of vertices 0 and 1, zw [H][W]; 0 where empty.
 * goi_texture_resolve: per pixel of a rasterization, uv (vt [n_vt][2] through ft [F][3]) and normal (vn [n_vn][3] through
 *   faces [F][3]) interpolated as (u a0 + v a1) + ((1 - u) - v) a2; n / sqrt(max(n.n, 1e-20)); viewcos = (n @ pose_rot)[2],
 *   pose_rot [3][3]; valid [HW] = tri > 0 and viewcos > 0.5; coords [HW][2] = clamp(uv, 0, 1)[[1, 0]] * 2 - 1 (0 where tri = 0);
 *   values [HW][3] = image [3][H][W] transposed.
 * goi_texture_grid_put: mipmap_linear_grid_put_2d(H, W, coords [N][2], values [N][C], min_resolution, return_count = True)
 *   without its early exit; valid [N] or NULL; 1 <= C <= GOI_TEXTURE_MAX_CHANNELS; N < 2^28.  Every texel sums its taps in
 *   ascending (tap 00 01 10 11, sample) order.  result [H][W][C], count [H][W].  acc / acc_count (both or neither): the view is
 *   also accumulated into them as goi_texture_accumulate does; norm_out / norm_mask (both or neither, and only with acc): what
 *   goi_texture_normalize gives for acc / acc_count after that, written by the same kernel.
 * goi_texture_accumulate: where cnt < 0.1: albedo += cur, cnt += cur_cnt (T texels).  goi_texture_normalize: mask = cnt > 0,
 *   out = albedo / cnt where mask, albedo elsewhere.
 * goi_texture_fill: a texel outside mask [h][w] with a mask texel within L1 distance `radius` (<= GOI_TEXTURE_MAX_RADIUS) takes
 *   albedo [h][w][C] of its nearest mask texel: the smallest (dx^2 + dy^2, row, column); nearest [h][w] = that texel's flat
 *   index, -1 elsewhere; out = albedo elsewhere.  h, w < 2^21. */
#define GOI_TEXTURE_STATUS_SORT 2   /* a look-back of a sort timed out on a wedged device: the results are garbage */
#define GOI_TEXTURE_STATUS_RANGE 8  /* an index outside its array: the face (or pixel) was treated as absent */
#define GOI_TEXTURE_MAX_CHANNELS 4
#define GOI_TEXTURE_MAX_RADIUS 127
#define GOI_TEXTURE_MAX_SIZE 16384
size_t goi_texture_rasterize_workspace_bytes(long long F, int H, int W);
int goi_texture_rasterize(long long V, long long F, const float* v_clip, const int* faces, int H, int W, int* tri, float* bary,
                          float* zw, int* status, void* workspace, void* stream);
int goi_texture_resolve(long long n_vt, long long n_vn, long long F, int H, int W, const int* tri, const float* bary,
                        const float* vt, const int* ft, const float* vn, const int* faces, const float* pose_rot,
                        const float* image, float* coords, float* values, unsigned char* valid, int* status, void* stream);
size_t goi_texture_grid_put_workspace_bytes(long long N, int C, int H, int W);
int goi_texture_grid_put(long long N, int C, int H, int W, int min_resolution, const float* coords, const float* values,
                         const unsigned char* valid, float* result, float* count, float* acc, float* acc_count, float* norm_out,
                         unsigned char* norm_mask, int* status, void* workspace, void* stream);
int goi_texture_accumulate(long long T, int C, float* albedo, float* cnt, const float* cur, const float* cur_cnt, void* stream);
int goi_texture_normalize(long long T, int C, const float* albedo, const float* cnt, float* out, unsigned char* mask,
                          void* stream);
size_t goi_texture_fill_workspace_bytes(int h, int w);
int goi_texture_fill(int h, int w, int C, int radius, const float* albedo, const unsigned char* mask, float* out, int* nearest,
                     void* workspace, void* stream);

/* ---- Rigid edits of a selection (csrc/edit.hip) -------------------------------------------------------------
 * x' = p + t + s R (x - p) applied IN PLACE to the selected rows of a model: what gui/main_edit.py:1512-1548 (obj_move) does for a
 * translation, extended by a rotation (covariances and SH bands 1..3 turn with the object) and a uniform scale.  Every pointer
 * is a device pointer; every entry point runs on `stream`, returns 0 (or -1: goi_raster_last_error) and never reads the device
 * back.  No float atomics: two calls give the same bits.  All float arithmetic is one fp32 rounding per operation, dot
 * products in index order.  selection [P] bytes (non-zero selects; with `invert` a zero byte does) or NULL = every row.
 *
 * goi_edit_bounds: over the selected rows of xyz [P][3]: *count, and out[12] = lo[3] (+inf when empty), hi[3] (-inf), centroid[3]
 *   (the float64 sum in a fixed order -- per-workgroup partials, then one fixed-order pass -- divided by the count and rounded
 *   once; 0 when empty), center[3] = 0.5 lo + 0.5 hi (0 when empty).  workspace: goi_edit_bounds_workspace_bytes(P) bytes (0: P
 *   out of range), 256-byte aligned.  0 <= P < 2^31.
 * goi_edit_transform: per selected row
 *     xyz       flags == 0: x + t (one add; R, s, pivot are not looked at).  Otherwise d = x - p, r_i = (R[i][0] d_0 + R[i][1] d_1)
 *               + R[i][2] d_2, x' = (s r + p) + t; p = pivot_dev[0..2] when pivot_dev is not NULL, else t->pivot.
 *     rotation  (raw (w, x, y, z), GOI_EDIT_ROTATE) q (x) r, the Hamilton product with q = t->q on the left, each component
 *               summed left to right.
 *     scaling   (raw log, GOI_EDIT_SCALE) + t->log_s.
 *     features_rest [P][M-1][3], M in {1, 4, 9, 16} (GOI_EDIT_ROTATE): band l = 1..3 of every channel is multiplied by D1 [3][3],
 *               D2 [5][5], D3 [7][7] (row-major): c'_i = sum_j D[i][j] c_j, j ascending.
 *   m_xyz, m_rotation, m_features_rest (each may be NULL; only with GOI_EDIT_ROTATE): Adam first moments of the same shapes, which
 *   get the linear part only: R m, q (x) m, D m.  A NULL parameter pointer is allowed where its flag is not set (and for
 *   features_rest with M == 1).  One launch. */
#define GOI_EDIT_ROTATE 1
#define GOI_EDIT_SCALE 2
typedef struct GoiEditTransform {
    float R[9];      /* row-major rotation */
    float q[4];      /* the same rotation as (w, x, y, z), unit */
    float t[3];
    float pivot[3];
    float s, log_s;
    int flags;       /* GOI_EDIT_* bits */
    float D1[9], D2[25], D3[49];
} GoiEditTransform;
size_t goi_edit_bounds_workspace_bytes(long long P);
int goi_edit_bounds(long long P, const float* xyz, const unsigned char* selection, int invert, int* count, float* out,
                    void* workspace, void* stream);
int goi_edit_transform(long long P, int M, const unsigned char* selection, int invert, const GoiEditTransform* t, float* xyz,
                       float* rotation, float* scaling, float* features_rest, float* m_xyz, float* m_rotation,
                       float* m_features_rest, const float* pivot_dev, void* stream);

/* ---- Pose gradients of a selection (csrc/pose.hip) ----------------------------------------------------------
 * The inverse of goi_edit_transform: the gradient of a loss with respect to the twist tau = (omega[3], t[3], sigma) of the
 * similarity x' = p + t + e^sigma Exp(omega) (x - p), r' = q(omega) (x) r, l' = l + sigma, c'_l = D_l(Exp(omega)) c_l applied to the
 * selected rows, at tau = 0, from the gradients a backward left for the raw parameters.  With d = x - p, r = (w, v), g_r = (g_w, g_v):
 *     out[0..2] = dL/domega = sum [ d x g_x  +  1/2 ((w g_v - g_w v) + v x g_v)  +  (sum_ch g_c[:, ch]^T G_k c[:, ch])_k ]
 *     out[3..5] = dL/dt     = sum g_x
 *     out[6]    = dL/dsigma = sum [ g_x . d  +  ((g_l0 + g_l1) + g_l2) ]
 * over the selected rows; *count = their number.  Minus the whole-model result is the gradient of moving the camera (omega, t only).
 *
 * goi_pose_gradient: P rows, 0 <= P < 2^31; M in {1, 4, 9, 16} SH coefficients (features_rest and g_features_rest [P][M-1][3]).
 *   selection [P] bytes (non-zero selects; with `invert` a zero byte does) or NULL = every row.  xyz [P][3], rotation [P][4] raw
 *   (w, x, y, z), features_rest: the parameters.  g_xyz, g_rotation, g_scaling [P][3], g_features_rest: their gradients; ANY may
 *   be NULL (not trained): its pieces are omitted and its parameter tensor is not read (scaling itself is never read).  Refused:
 *   all four NULL (with P > 0), a gradient whose parameter is NULL, g_features_rest with M = 1, NULL out / count / generators, a
 *   NULL or misaligned workspace.  generators: HOST pointer to the 48 non-zero entries of the SH rotation generators G_x (18),
 *   G_y (18), G_z (12) over bands 1..3, row-major within each (pose.py: sh_generators, generator_entries); where they sit is
 *   compiled in.  pivot_host: HOST float[3] (NULL: the origin), used unless pivot_dev (device float[3]) is given.  out: device
 *   double[7]; count: device int[1].  workspace: goi_pose_gradient_workspace_bytes(P) bytes (0: P out of range), 256-byte aligned.
 *   Every piece of a row is formed in fp32, one rounding per operation, as written above with d first (products before their sum,
 *   dot products in index order, the entries of a generator left to right); each piece -- three for omega, two for sigma, g_x for
 *   t -- is converted to double and summed in float64 in a fixed order: per thread over its rows, the wave butterfly, the waves in
 *   order, then at most 1024 per-workgroup partials by one workgroup in the same way.  No float atomics: two calls give the same
 *   bits.  P = 0 or an empty selection gives zeros and count 0.  Two launches on `stream`, no read-back; returns 0 (or -1:
 *   goi_raster_last_error). */
size_t goi_pose_gradient_workspace_bytes(long long P);
int goi_pose_gradient(long long P, int M, const unsigned char* selection, int invert, const float* xyz, const float* rotation,
                      const float* features_rest, const float* g_xyz, const float* g_rotation, const float* g_scaling,
                      const float* g_features_rest, const float* generators, const float* pivot_host, const float* pivot_dev,
                      int* count, double* out, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
