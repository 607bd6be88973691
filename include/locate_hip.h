/* locate_hip.h - C ABI of the MI355X (gfx950) kernels for the LocAtE generator/discriminator training step.
 *
 * The reference (ClashLuke/LocAtE) has no FFI: its operator boundary is the Python autograd.Function /
 * nn.Module protocol.  Each entry point below replaces the arithmetic of one
 * reference operator (cited per function as file:line in the reference tree) and is what a ctypes stub in
 * the reference would bind.
 *
 * Conventions
 *   - all data pointers are DEVICE pointers to fp32, NCHW, contiguous unless a batch stride is given;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); calls are asynchronous;
 *   - every function returns 0 on success, non-zero on error (1 = bad argument, 2 = launch failure) and
 *     never throws; locate_last_error() returns a thread-local message for the last failure;
 *   - the library never allocates: outputs and workspaces are owned by the caller; the *_workspace_bytes
 *     helpers give the required sizes; workspaces may be reused by the next call on the same stream;
 *   - entry points are stateless and re-entrant (forward on the caller's thread, backward on the autograd
 *     worker thread, each with its own stream).
 */
#ifndef LOCATE_HIP_H
#define LOCATE_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

const char* locate_last_error(void);
int locate_abi_version(void);
/* architecture name ("gfx950..."), compute units and wavefront size of the current device */
int locate_device_info(char* arch_name, int name_len, int* cu_count, int* wave_size);

/* ---- RootTanh: y = (x^2+1)^(1/4) tanh x and its hand-written derivative (libs/activation.py:7-36) ---- */
int locate_roottanh_fwd(const float* x, float* y, int64_t n, void* absmax /* nullable, see locate_roottanh_bwd */, void* stream);
/* accumulate: gx +=.  absmax (nullable): locate_absmax_words() (= 1024: 32 words in use, one per 128-byte line) device words,
 * ZERO before the call; the kernel folds the largest |gx| into them (atomic max on the bit pattern - order-independent - spread
 * over cache lines so that a few thousand blocks do not queue on one; the tensor's maximum is the maximum of the words) for a
 * contraction that consumes gx in its fp16-piece form (precision 2 below) */
int locate_absmax_words(void);
int locate_roottanh_bwd(const float* x, const float* gy, float* gx, int64_t n, int accumulate, void* absmax, void* stream);
/* the same word for any tensor (tests, tools, weights packed outside an optimizer step) */
int locate_absmax(const float* x, int64_t n, void* absmax, void* stream);
/* generator output tanh (libs/models.py:66); backward takes the forward OUTPUT y */
/* style chain link (libs/block.py:119-125): out[r, :z] = latent[r, :], out[r, z:] = RootTanh(pre[r, :]) in one launch, and
 * its backward on the gradient's column slice in place (row stride in elements) */
int locate_act_cat_rows_fwd(const float* latent, const float* pre, float* out, int rows, int z, int w, void* stream);
/* g_add (nullable, [rows, w] contiguous): added to the result - the gradient pre receives as a norm's style scale */
int locate_act_rows_bwd(const float* pre, const float* g, int64_t g_row_stride, const float* g_add, float* gpre, int rows, int w,
                        void* stream);
/* out = (a + b) + c, each operand contiguous inside a batch element with its own batch stride (elements): the one-pass sum of
 * the three gradients that meet at a discriminator block's input (libs/block.py:38-52, libs/scale.py:28-34: the conv branch's
 * norm, the identity half of the concatenation, the skip branch's 1x1 conv) - the reference leaves two adds to autograd */
int locate_add3(const float* a, int64_t a_bs, const float* b, int64_t b_bs, const float* c, int64_t c_bs, float* out, int batch,
                int64_t per, void* stream);
int locate_tanh_fwd(const float* x, float* y, int64_t n, void* stream);
int locate_tanh_bwd(const float* y, const float* gy, float* gx, int64_t n, void* stream);

/* ---- InPlaceNorm: global scalar mean / unbiased std, per-channel or per-sample scale, per-channel bias
 *      (libs/inplace_norm.py:4-45).  stats = {mean, std}. ---- */
size_t locate_norm_stats_workspace_bytes(void);
int locate_norm_stats(const float* x, int64_t n, float* stats, void* workspace, void* stream);
/* fused forward in two launches (statistics + apply): out = (x - mean) * scale / std + bias; scale is [C]
 * (scale_per_sample = 0) or [B*C]; with_act = 1 stores RootTanh(out) INSTEAD of out (the conv stage that follows starts
 * with RootTanh, libs/conv.py:22-24).  groups > 1: the batch stacks `groups` independent forward calls of B/groups
 * samples each (the three discriminator passes of main.py:149-152), every one with its OWN mean/std.
 * stats_out = groups x {mean, std}; workspace: locate_norm_stats_workspace_bytes() */
/* pre_partial (nullable): statistics partials of x already produced by the kernel that wrote x (locate_gate_fwd_stats with
 * the same group count); the statistics pass over x is then skipped */
int locate_norm_fwd(const float* x, const float* scale, int scale_per_sample, const float* bias, float* out, int with_act,
                    float* stats_out, int B, int C, int hw, int groups, void* workspace, const double* pre_partial,
                    void* absmax /* nullable: largest |out|, see locate_roottanh_bwd */, void* stream);
size_t locate_norm_bwd_workspace_bytes(int B, int C);
/* full backward incl. the path through std (libs/inplace_norm.py:17-27 + ATen std backward); with_act = 1: g is the
 * gradient w.r.t. RootTanh(out) and RootTanh' (libs/activation.py:22-36) is applied from the recomputed out;
 * dscale / dbias sum over all groups (the reference accumulates the three passes' gradients, main.py:153-157) */
/* accumulate_dx / accumulate (locate_norm_bwd, locate_gate_bwd, locate_feature_pool_bwd): add into the output instead of
 * overwriting it - the second consumer of a forked tensor completes the gradient the first one started (ops.fork) */
int locate_norm_bwd(const float* x, const float* g, const float* stats, const float* scale, int scale_per_sample,
                    const float* bias, int with_act, float* dx, float* dscale, float* dbias, int B, int C, int hw, int groups,
                    void* workspace, int accumulate_dx, void* stream);
/* out[c] = sum over batch and space of g[b, c, :] (bias gradients: libs/scale.py:28-34, libs/linear.py:10) */
/* the same backward in TWO launches (no middle launch in the pass's dependent chain): dx and - with scale_per_sample - the
 * per-sample scale gradient; the per-channel dscale[c] / dbias[c] (parameter gradients) come from locate_fin_norm_channels at
 * the end of the pass, out of the plane sums S1, S2 this call leaves in its workspace at locate_norm_bwd_fused_plane_offset()
 * (S1 [B*C] floats, then S2): records p = {S1, S2, stats, dscale [C] | 0, dbias [C] | 0}, i = {B, C, groups} */
size_t locate_norm_bwd_fused_workspace_bytes(int B, int C);
size_t locate_norm_bwd_fused_plane_offset(void);
int locate_norm_bwd_fused(const float* x, const float* g, const float* stats, const float* scale, int scale_per_sample,
                          const float* bias, int with_act, float* dx, float* dscale_sample, int B, int C, int hw, int groups,
                          void* workspace, int accumulate_dx, void* stream);
/* the plane pass of locate_norm_bwd_fused alone (S1 / S2, dscale_sample and the per-block group sums as that call leaves them):
 * dx is formed by the kernel that consumes it, locate_gate_bwd_term, from the first locate_norm_bwd_fused_partials(B, C) block
 * records at the start of `workspace` */
int locate_norm_bwd_fused_partials(int B, int C);
int locate_norm_bwd_planes(const float* x, const float* g, const float* stats, const float* scale, int scale_per_sample,
                           const float* bias, int with_act, float* dscale_sample, int B, int C, int hw, int groups,
                           void* workspace, void* stream);
int locate_fin_norm_channels(const void* records, int n, void* stream);
size_t locate_channel_sum_workspace_bytes(int B, int C, int hw);
int locate_channel_sum(const float* g, float* out, int B, int C, int hw, int64_t batch_stride, void* workspace, void* stream);

/* ---- residual gate out = (gamma a + 1) x (libs/merge.py:19-62), incl. dgamma = sum x^2 g as coded.
 *      a_per_plane = 1: `a` holds one value per (batch, channel) plane (stride-0 expand, libs/util_modules.py:6-12) */
int locate_gate_fwd(const float* x, const float* a, int a_per_plane, const float* gamma, float* out, int64_t planes, int hw,
                    void* stream);
/* the same gate plus, from its epilogue, the InPlaceNorm statistics partials (sum, sum of squares per block, fp64) of `out`
 * for `groups` calls stacked along the batch: stats_partial = locate_norm_stats_workspace_bytes() bytes, handed to
 * locate_norm_fwd as pre_partial (libs/block.py:44-52: a gate's output is what the next norm normalises) */
int locate_gate_fwd_stats(const float* x, const float* a, int a_per_plane, const float* gamma, float* out, int64_t planes,
                          int hw, int groups, double* stats_partial, void* stream);
size_t locate_gate_bwd_workspace_bytes(int64_t planes);
/* dgamma nullable: the kernel then only leaves its locate_gate_bwd_partials(planes, hw) block sums (doubles, at the start of
 * `workspace`; dgamma = their sum in index order) for the caller to add up - see locate_fin_sums - or to ignore */
int locate_gate_bwd_partials(int64_t planes, int hw);
int locate_gate_bwd(const float* x, const float* a, int a_per_plane, const float* gamma, const float* g, float* dx, float* da,
                    float* dgamma, int64_t planes, int hw, void* workspace, int accumulate_dx,
                    void* da_absmax /* nullable: largest |da| (full-map form), see locate_roottanh_bwd */, void* stream);
/* The same backward with the gradient w.r.t. the gate's output FORMED inside the kernel instead of read from g - the gate's
 * output out = (gamma a + 1) x is recomputed bit for bit, so the element-wise launch that would have produced g, and its pass
 * over the tensor, go away.  Same results, bit for bit, as the two calls it replaces.
 *   LOCATE_GATE_TERM_NONE      locate_gate_bwd
 *   LOCATE_GATE_TERM_NORM      out fed an InPlaceNorm whose backward ran its plane pass only (locate_norm_bwd_planes with the
 *                              same B, C, hw, groups; B * C == planes): the gradient is that norm's dx from go, stats, scale,
 *                              bias and the first npartial = locate_norm_bwd_fused_partials(B, C) records of its workspace
 *                              (`partial`), plus g where has_share says that another consumer of out left its share there
 *                              (dx + share, locate_norm_bwd_fused's accumulate order); g is not read otherwise
 *   LOCATE_GATE_TERM_ROOTTANH  out fed a RootTanh: the gradient is RootTanh'(out) g (locate_roottanh_bwd) */
enum { LOCATE_GATE_TERM_NONE = 0, LOCATE_GATE_TERM_NORM = 1, LOCATE_GATE_TERM_ROOTTANH = 2 };
typedef struct {
    int32_t kind, with_act, per_sample, has_share;
    const float* go;
    const float* stats;
    const float* scale;
    const float* bias;
    const double* partial;
    int32_t npartial, B, C, groups;
} LocateGateTerm;
int locate_gate_bwd_term(const float* x, const float* a, int a_per_plane, const float* gamma, const float* g, float* dx, float* da,
                         float* dgamma, int64_t planes, int hw, void* workspace, int accumulate_dx, void* da_absmax,
                         LocateGateTerm term, void* stream);

/* ---- softmax over the last dimension of [rows, n] (libs/attention.py:35,47) ---- */
int locate_softmax_fwd(const float* x, float* y, int64_t rows, int n, void* stream);
int locate_softmax_bwd(const float* y, const float* gy, float* gx, int64_t rows, int n, void* stream);

/* ---- skip-branch resampling / indexing (libs/scale.py:7-45, libs/merge.py:4-16) ---- */
int locate_upsample2x_fwd(const float* x, float* y, int64_t planes, int H, int W, void* stream);   /* bilinear, align_corners=False */
int locate_upsample2x_bwd(const float* gy, float* gx, int64_t planes, int H, int W, void* stream);
/* FeaturePooling(r = 2) followed by the x2 upsample - the generator's skip branch (libs/scale.py:7-16,37-38) - in ONE launch:
 * x is the RAW tensor of 2 * planes * H * W elements (FeaturePooling averages ADJACENT FLAT elements), y: [planes, 2H, 2W];
 * bit for bit locate_feature_pool_fwd(r = 2) + locate_upsample2x_fwd.  _bwd: the adjoint, gx = the raw gradient (accumulate != 0:
 * added to what gx holds - the second consumer of a forked tensor, as in locate_feature_pool_bwd). */
int locate_pool2_upsample2x_fwd(const float* x, float* y, int64_t planes, int H, int W, void* stream);
int locate_pool2_upsample2x_bwd(const float* gy, float* gx, int64_t planes, int H, int W, int accumulate, void* stream); /* H, W: forward input size */
int locate_avgpool2_fwd(const float* x, float* y, int64_t planes, int H, int W, void* stream);
int locate_avgpool2_bwd(const float* gy, float* gx, int64_t planes, int H, int W, int accumulate, void* stream);   /* H, W: forward input size */
int locate_feature_pool_fwd(const float* x, float* y, int64_t n_out, int r, void* stream);         /* mean of r adjacent flat elements */
int locate_feature_pool_bwd(const float* gy, float* gx, int64_t n_out, int r, int accumulate, void* stream);
/* dst[b, c, :] (+)= src[b, c, :], c < C, independent batch strides (torch.cat along channels and its backward) */
int locate_copy_channels(const float* src, float* dst, int B, int C, int hw, int64_t src_batch_stride,
                         int64_t dst_batch_stride, int accumulate, void* stream);

/* ---- spectral norm state machine (libs/spectral_norm.py:21-32): one power iteration, u/v updated in place,
 *      sigma = {sigma, 1/sigma}, wv = W v (kept for du).  W_bar viewed as [h, wd], h = shape[0]. ---- */
size_t locate_sn_workspace_bytes(int h, int wd);
int locate_sn_power_iter(const float* w, float* u, float* v, float* sigma, float* wv, int h, int wd, void* workspace,
                         void* stream);
/* all layers of a network in four launches; `table`: device array of records {w,u,v,sigma,wv,t,s,tpart pointers;
 * int h, wd, nchunk, pad} (locate_sn_table_record_bytes() each), scratch t[wd], s[h], tpart[ceil(h/64)*wd] */
size_t locate_sn_table_record_bytes(void);
int locate_sn_power_iter_batched(const void* table, int n_layers, int max_h, int max_wd, void* stream);
/* after locate_conv_wgrad(.., w_ref = W_bar, inv_scale = 1/sigma, inner_partial): gw (in/out) enters as G/sigma and
 * leaves as dW_bar = G/sigma + dsigma u v^T with dsigma = -<G, W_bar>/sigma^2; du = dsigma (W v) (nullable);
 * dsigma_out[0] = dsigma (nullable).  u, v are the CURRENT state (the reference's autograd sees the latest .data). */
int locate_sn_weight_bwd(const double* inner_partial, int n_partial, const float* u, const float* v, const float* sigma,
                         const float* wv, float* gw, float* du, float* dsigma_out, int h, int wd, void* stream);
/* the same for `groups` (<= 4) forward calls stacked along the batch of ONE layer call, each with its own sigma_k, v_k
 * (the reference runs them one after the other, main.py:149-152): gw enters as sum_k G_k/sigma_k (locate_conv_wgrad
 * with group scaling); dsigma_k = -<gy_k, y_k - bias>/sigma_k  (= -<G_k, W_bar>/sigma_k^2 taken on the activation side);
 * gw += (sum_k dsigma_k) u v^T; du = sum_k dsigma_k W v_k; dsigma_total_out = sum_k dsigma_k.
 * sigma_tab: {sigma_k, 1/sigma_k} pairs sigma_stride floats apart; wv rows wv_stride floats apart. */
size_t locate_sn_group_workspace_bytes(void);
int locate_sn_weight_bwd_grouped(const float* gy, int64_t gy_bs, const float* y, int64_t y_bs, const float* bias, int groups,
                                 int Bg, int M, int plane, const float* sigma_tab, int sigma_stride, const float* u,
                                 const float* v, const float* wv, int64_t wv_stride, float* gw, float* du,
                                 float* dsigma_total_out, int h, int wd, void* workspace, void* stream);
/* dv = (sum of the layer's 4 dsigma slots) * W^T u for all layers of `table` (records as for
 * locate_sn_power_iter_batched; field v = dv output, field sigma = the 4 slots, cleared afterwards) */
int locate_sn_dv_batched(const void* table, int n_layers, int max_h, int max_wd, void* stream);

/* ---- dense contractions as implicit GEMMs on the fp32 MFMA (libs/conv.py:14-20, libs/attention.py:18-46,
 *      libs/scale.py:25-34, libs/linear.py:10).  geom = {B, C, H, W, M, KH, KW, stride, pad_h, pad_w, OH, OW}
 *      describes the REGULAR convolution R: out[b,m,oh,ow] = sum w[m,c,kh,kw] in[b,c,oh*s-ph+kh,ow*s-pw+kw].
 *      The weight operand is a pre-packed K-major panel (locate_conv_pack_panel; redo only when W changes);
 *      `scale` (nullable device scalar) multiplies the contraction in the epilogue (1/sigma of spectral norm,
 *      libs/spectral_norm.py:31-32); *_bs are batch strides in elements; workspace = split-K slabs (may be 0). ---- */
size_t locate_conv_panel_bytes(const int* geom, int adjoint);
int locate_conv_pack_panel(const int* geom, int adjoint, const float* w, float* panel, void* stream);
/* all panels of a network in one launch (after an optimizer step): one HOST record of locate_conv_pack_job_bytes()
 * per panel, filled by locate_conv_pack_job (block_start = running sum of *blocks_out), uploaded by the caller */
size_t locate_conv_pack_job_bytes(void);
/* direct != 0: RE-packing of a panel that has been packed in full before, in one pass (piece planes straight from the weights,
 * fp32 rows only where a kernel reads them).  fp16-piece panels need weight_absmax for it: locate_absmax_words() device words
 * with the largest magnitude of w as it is now (locate_nadam_step leaves them per tensor); else the two-pass form is taken */
int locate_conv_pack_job(const int* geom, int adjoint, const float* w, float* panel, int block_start, void* job_out,
                         int* blocks_out, int direct, const void* weight_absmax);
/* any_f16: some job is a non-direct fp16-piece panel (its absmax header is cleared first); passes: bit 0 = some gather-kernel
 * panel is in the two-pass form (split launch), bit 1 = some WINDOW panel of fp16 pieces came without absmax words (absmax
 * pre-pass into the panel headers); both 0 when every job took the direct form (locate_conv_pack_job_is_direct): one launch */
int locate_conv_pack_panels(const void* jobs, int n_jobs, int total_blocks, int any_f16, int passes, void* stream);
int locate_conv_pack_job_is_direct(const void* job);
int locate_conv_pack_job_is_window(const void* job);
/* ---- window form of the dense contractions (csrc/convwin.hip): the gathered operand is staged in LDS once per block and 8
 *      reduction channels as the raw window of the map its 128 output columns see, every tap's MFMA fragment is read from that
 *      one image (libs/conv.py:14-20's k x k convs, both directions; the 1x1 contractions of libs/scale.py:25-34,
 *      libs/attention.py:44-46).  locate_conv_win_ok(geom, adjoint | fmt, x_bs, x): 1 when this geometry / direction / operand
 *      alignment has the form.  The caller then uses panel format bit 2 (`adjoint | fmt | 4`) in locate_conv_panel_bytes /
 *      _pack_panel / _pack_job, passes `precision | 16` to locate_conv_fwd / locate_conv_dgrad and sizes the split-K workspace
 *      with locate_conv_win_workspace_bytes.  Same arithmetic and accuracy as the gather kernels at each precision. ---- */
int locate_conv_win_ok(const int* geom, int adjoint_fmt, int64_t x_bs, const void* x);
size_t locate_conv_win_workspace_bytes(const int* geom, int adjoint_fmt);
size_t locate_conv_fwd_workspace_bytes(const int* geom);
/* arrival counters for split-K launches that combine their partial tiles INSIDE the launch (the tile's last-arriving block
 * sums them in a fixed order: bit-reproducible): locate_conv_counter_bytes() bytes of device memory, zero before their first
 * use, left zero by every completed call, never shared by launches that may run concurrently (one block per layer and
 * direction is what the Python layer keeps).  `counters` may be NULL: a second kernel then sums the partial tiles. */
size_t locate_conv_counter_bytes(void);
/* scale_group_batch = 0: `scale` is one scalar; > 0: batch element b uses scale[(b / scale_group_batch) * scale_stride].
 * precision (locate_conv_fwd / _dgrad / _wgrad): 0 = fp32-faithful products (the reference's arithmetic: both operands split
 * exactly into three bf16 pieces, six bf16 MFMAs per slice, fp32 accumulation); 1 = bf16 operands (both operands rounded to
 * nearest-even bf16, one MFMA per slice, fp32 accumulation and fp32 storage) - the mixed-precision variant BASELINE.json
 * configs[1] names; tolerance against the fp32 path stated in tests/test_gpu_bf16.py. */
/* Placement contract of every contraction (locate_conv_*, locate_dwconv_*, locate_groupdot_*): its results depend on the elements
 * of its own operands only, and it writes the elements of its own outputs only, wherever those lie - an operand or output may be
 * a channel slice of a wider NCHW tensor (dense [C, H, W] planes, any batch stride >= one sample) that starts on any fp32
 * element; what lies between the images of a view and around it is neither read into a result (not even against a zero weight)
 * nor written.  Where a route needs more than 4-byte alignment it either takes another kernel (the pointwise stream, the window
 * form, the paired-load weight-gradient kernels, the vector bodies of the reductions) or refuses the call with status 1 before
 * anything is launched (locate_conv_wgrad on its narrow 1x1 route and its 192-row plan: locate_conv_wgrad_operand_align; the
 * window form: locate_conv_win_ok).  tests/test_gpu_contraction_views.py; the table is DESIGN.md, "Pointer alignment". */
int locate_conv_fwd(const int* geom, const float* x, int64_t x_bs, const float* panel, const float* scale,
                    int scale_group_batch, int scale_stride, const float* bias, float* y, int64_t y_bs, void* workspace,
                    void* counters, int precision, const void* x_absmax, const void* act_epilogue, void* stream);
/* act_epilogue (nullable): HOST pointer to
 *   struct { void* act_out; int64_t act_bs; const void* lat; int64_t lat_bs; int32_t lat_z, pad;
 *            const void* mul_pre; int64_t mul_bs; void* out_absmax; }
 * act_out: the launch also writes act_out[b, m, pixel] = RootTanh(y[b, m, pixel]) (batch stride act_bs elements) - the
 *   activation between the two convs of a stage (libs/conv.py:19-20, libs/attention.py:44-46, libs/linear.py:12-13) without a
 *   launch and a read of its own; on 1x1 maps, with lat, it copies lat[n, 0 .. lat_z) in front of row n
 *   (act_out[n * act_bs - lat_z ..]): the next style link's input cat([latent, activated]) (libs/block.py:119-125).
 * mul_pre (locate_conv_dgrad; excludes act_out): the contraction's result is multiplied by RootTanh'(mul_pre[b, c, pixel])
 *   (batch stride mul_bs) before it is stored - the input gradient of a conv whose input was RootTanh(mul_pre) leaves the launch
 *   as the gradient of mul_pre itself (the separate locate_roottanh_bwd launch and its read of gx disappear).
 * out_absmax (nullable): locate_absmax_words() zeroed words that receive the largest magnitude of act_out (of gx with mul_pre). */
/* precision: 0 = fp32-faithful with three bf16 pieces per operand (six bf16 MFMAs per 32x32x16 slice); 1 = operands rounded
 * to bf16 (one MFMA); 2 = fp32-faithful with TWO fp16 pieces per operand (three fp16 MFMAs): both operands are scaled by a
 * power of two into fp16's range - the weights when the panel is packed (panel format bit: `adjoint | 2` in
 * locate_conv_panel_bytes / locate_conv_pack_panel / locate_conv_pack_job), the gathered tensor inside the kernel from
 * *x_absmax, the bit pattern of its largest magnitude (locate_absmax, or the absmax outputs of the producing kernels) - and
 * the exact inverse factors are applied to the accumulators.  Same fp32-level accuracy as precision 0 (tools/bench_conv.py
 * --check), half the matrix instructions. */
/* data adjoint of R (= ConvTranspose2d forward with weight [C_in = M, C_out = C, KH, KW]); panel: adjoint = 1 */
size_t locate_conv_dgrad_workspace_bytes(const int* geom);
int locate_conv_dgrad(const int* geom, const float* gy, int64_t gy_bs, const float* panel, const float* scale,
                      int scale_group_batch, int scale_stride, const float* bias, float* gx, int64_t gx_bs, void* workspace,
                      void* counters, int precision, const void* gy_absmax, const void* act_epilogue, void* stream);
/* gw[m,c,kh,kw] = inv_scale * sum_{b,oh,ow} gy[b,m,oh,ow] x[b,c,oh*s-ph+kh,ow*s-pw+kw] (deterministic split reduction).
 * With w_ref (= W_bar) and inner_partial the same pass emits locate_conv_wgrad_partials(geom) partial sums (double)
 * of <UNSCALED gw, W_bar>, which the spectral-norm backward needs; inv_scale, w_ref, inner_partial are nullable.
 * scale_group_batch > 0: gy of batch element b is weighted by inv_scale[(b / scale_group_batch) * scale_stride] instead
 * (gw = sum_k G_k / sigma_k over stacked forward calls; <= 4 groups; w_ref and inner_partial must be null). */
/* (layers with M % 192 == 0 on maps with even OH * OW and OW run on 192 x 128 tiles of the paired-load kernels only: gy must then
 * be 8-byte aligned with an even batch stride - any contiguous tensor is) */
size_t locate_conv_wgrad_workspace_bytes(const int* geom);
int locate_conv_wgrad_partials(const int* geom);
/* bytes that the address and the batch stride of x (which = 0) / gy (which = 1) must be a multiple of for locate_conv_wgrad to
 * take them at this geometry: 16 (narrow 1x1 route, both), 8 (gy on the 192-row plan) or 4; anything else is refused there */
int locate_conv_wgrad_operand_align(const int* geom, int which);
/* deferred_reduce (nullable; host memory, locate_slab_reduce_record_bytes() bytes): the split reduction of this launch is not
 * run but written there; gw / inner_partial are complete after locate_slab_reduce_batch() has run the record (at most
 * locate_slab_reduce_max() records per call; the workspace stays untouched until then).  locate_slab_reduce_record_blocks() == 0:
 * the geometry has no split reduction, nothing is pending.  One launch then finishes ALL weight gradients of a backward pass. */
int locate_conv_wgrad(const int* geom, const float* x, int64_t x_bs, const float* gy, int64_t gy_bs, float* gw,
                      const float* w_ref, const float* inv_scale, int scale_group_batch, int scale_stride,
                      double* inner_partial, void* workspace, int precision, const void* x_absmax, const void* gy_absmax,
                      void* deferred_reduce, void* stream);
/* Stacked calls (scale_group_batch > 0) WITH w_ref + inner_partial: the split reduction is laid out so that no slab crosses a
 * call boundary and emits the partial sums of <G_k / sigma_k, W_bar> per call - inner_partial[call][partial], groups x
 * locate_conv_wgrad_group_partials(geom, groups) doubles, workspace of locate_conv_wgrad_group_workspace_bytes(geom, groups) bytes.
 * Their sum over the partials equals <gy_k, y_k - bias> (locate_fin_sn_dots), without reading gy and y again.  0 partials: this
 * geometry cannot (1x1 maps, one output pixel, call lengths that do not divide into whole slabs) - use locate_fin_sn_dots. */
int locate_conv_wgrad_group_partials(const int* geom, int groups);
size_t locate_conv_wgrad_group_workspace_bytes(const int* geom, int groups);
size_t locate_slab_reduce_record_bytes(void);
int locate_slab_reduce_max(void);
int locate_slab_reduce_record_blocks(const void* record);
int locate_slab_reduce_batch(const void* records, int n, void* stream);

/* The weight gradients of ALL small-map layers of one backward pass in ONE launch: the style chain's linears
 * (libs/linear.py:7-15, libs/block.py:112-127), the channel gates' squeeze convs, the discriminator's layers on 1x1 maps, its
 * last 5x5 conv and its head (one output pixel) - in the reference ~19 separate autograd weight-gradient kernels per iteration.
 * locate_wgrad_batch_record() writes the launch of locate_conv_wgrad for one layer into a host record (same argument meaning)
 * and returns its block count, or 0 when the geometry is not such a layer (launch it with locate_conv_wgrad then);
 * locate_wgrad_batch() runs up to locate_wgrad_batch_max() packed records; results are those of the single launches. */
size_t locate_wgrad_batch_record_bytes(void);
int locate_wgrad_batch_max(void);
int locate_wgrad_batch_record(const int* geom, const float* x, int64_t x_bs, const float* gy, int64_t gy_bs, float* gw,
                              const float* w_ref, const float* inv_scale, int scale_group_batch, int scale_stride,
                              double* inner_partial, void* record);
int locate_wgrad_batch(const void* records, int n, void* stream);

/* ---- grouped convolutions of the SEPARABLE switch (libs/config.py:53; replaces the torch.nn.Conv2d /
 *      ConvTranspose2d(groups = ...) forward + autograd backward under libs/conv.py:14-18 and libs/attention.py:15-21).
 *      Depthwise: geom as above describes the REGULAR depthwise conv R between a "big" side [B, C, H, W] and a "small"
 *      side [B, M, OH, OW]; the side with more channels has one weight row [KH*KW] per channel, the other side has
 *      1/mult as many channels (channel o of the wide side pairs with channel o / mult of the narrow side):
 *        Conv2d(C, C*mult, groups=C)           forward = dwconv_fwd   (M = C*mult), input gradient = dwconv_dgrad
 *        ConvTranspose2d(M, M*mult, groups=M)  forward = dwconv_dgrad (C = M*mult), input gradient = dwconv_fwd
 *      w is the layer's weight tensor as stored (no packing).  scale / scale_group_batch / scale_stride as in locate_conv_fwd. ---- */
int locate_dwconv_fwd(const int* geom, const float* x, int64_t x_bs, const float* w, const float* scale, int scale_group_batch,
                      int scale_stride, float* y, int64_t y_bs, void* stream);
int locate_dwconv_dgrad(const int* geom, const float* gy, int64_t gy_bs, const float* w, const float* scale,
                        int scale_group_batch, int scale_stride, float* gx, int64_t gx_bs, void* stream);
/* gw[row, kh, kw] = inv_scale * sum_{b,oh,ow} small[b, row or row/mult, oh, ow] big[b, row/mult or row, oh*s-ph+kh, ow*s-pw+kw]
 * (deterministic two-stage reduction; square kernels up to 5 x 5).  w_ref / inner_partial / per-call scales as in
 * locate_conv_wgrad; locate_dwconv_wgrad_partials(geom) doubles are written. */
size_t locate_dwconv_wgrad_workspace_bytes(const int* geom);
int locate_dwconv_wgrad_partials(const int* geom);
int locate_dwconv_wgrad(const int* geom, const float* big, int64_t big_bs, const float* small, int64_t small_bs, float* gw,
                        const float* w_ref, const float* inv_scale, int scale_group_batch, int scale_stride,
                        double* inner_partial, void* workspace, void* stream);
/* Conv2d(G*cpg, G, kernel = the whole S x S map, groups = G) (libs/attention.py:15-21): y[b, g] = scale * <w[g, :], x[b, g, :]>
 * over L = cpg*S*S contiguous elements; x [B, G*L] with batch stride x_bs, w [G, L], y / gy [B, G] dense. */
int locate_groupdot_fwd(const float* x, int64_t x_bs, const float* w, const float* scale, int scale_group_batch,
                        int scale_stride, float* y, int B, int G, int L, void* stream);
int locate_groupdot_dgrad(const float* gy, const float* w, const float* scale, int scale_group_batch, int scale_stride,
                          float* gx, int64_t gx_bs, int B, int G, int L, void* stream);
int locate_groupdot_wgrad_partials(int G, int L);
int locate_groupdot_wgrad(const float* x, int64_t x_bs, const float* gy, float* gw, const float* w_ref, const float* inv_scale,
                          int scale_group_batch, int scale_stride, double* inner_partial, int B, int G, int L, void* stream);

/* ---- end-of-backward finalisers, batched over all layers of a backward pass (finalise.hip): what only feeds PARAMETER
 *      gradients - spectral norm's rank-1 term with du / dsigma (libs/spectral_norm.py:31-32 under autograd), the stacked
 *      calls' <gy_k, y_k - bias>, the gates' dgamma sums (libs/merge.py:33-38) - in one launch per kind instead of two or
 *      three small launches per layer.  `records`: HOST array of n records of locate_fin_record_bytes() = 112 bytes
 *      { const void* p[8]; int64 l[2]; int32 i[8]; } passed on BY VALUE in the kernel arguments (no device table):
 *        dots : p = {gy, y, bias|0, partial out [groups][np]}, l = {gy_bs, y_bs}, i = {groups, Bg, M, plane};
 *               np = locate_fin_sn_dot_partials(Bg, M, plane)
 *        rank1: p = {partial (double), sigma table, u, v, wv, gw (in/out), du|0, dsigma_out|0}, l = {wv_stride},
 *               i = {npartial per call, groups (0 = one call: locate_sn_weight_bwd's arithmetic; k >= 1 = stacked:
 *               locate_sn_weight_bwd_grouped's), sigma_stride, h, wd}
 *        sums : p = {partials (double), out (float)}, i = {count}
 *      Same arithmetic and summation order as the per-layer entry points: bit-identical results. ---- */
size_t locate_fin_record_bytes(void);
int locate_fin_sn_dot_partials(int Bg, int M, int plane);
int locate_fin_sn_dots(const void* records, int n, void* stream);
int locate_fin_sn_rank1(const void* records, int n, void* stream);
int locate_fin_sums(const void* records, int n, void* stream);
/* channel sums out[c] = sum_{b,hw} g[b,c,hw] (bias gradients: libs/scale.py:28-34, libs/linear.py:10) for all biases of a pass:
 * records p = {g, out [C], partials [slices][C] | 0}, l = {batch stride}, i = {B, C, hw}; slices = locate_fin_channel_slices */
int locate_fin_channel_slices(int B, int C, int hw);
int locate_fin_channel_sums(const void* records, int n, void* stream);

/* ---- gradient bucket pack / unpack of the data-parallel exchange (no reference counterpart: libs/config.py:10-11 is single
 *      device).  tensors: DEVICE array of {float* grad; float* flat; int64 n} records (locate_multi_copy_record_bytes() = 24);
 *      chunks: DEVICE (tensor index, chunk index) int pairs in pieces of locate_multi_copy_chunk_elems();
 *      direction 0: flat <- grad;  1: grad <- flat * scale ---- */
size_t locate_multi_copy_record_bytes(void);
int locate_multi_copy_chunk_elems(void);
int locate_multi_copy(const void* tensors, const void* chunks, int n_chunks, int direction, float scale, void* stream);

/* ---- fused multi-tensor Nadam (libs/nadam.py:31-89); per-tensor (step, m_schedule) state lives on device ---- */
size_t locate_nadam_tensor_record_bytes(void);   /* {float* p; const float* g; float* m; float* v; double* sched; int64 n;
                                                     uint32* absmax (nullable: locate_absmax_words() words, receive max |p| after the step)} */
int locate_nadam_chunk_elems(void);
int locate_nadam_step(const void* tensors, void* coef, const void* chunks, int n_tensors, int n_chunks, double lr, double beta1,
                      double beta2, double eps, double schedule_decay, double weight_decay, void* stream);

/* ---- exponential moving average of a network's weights (no reference counterpart), every tensor in one launch.
 *      tensors: DEVICE array of {float* avg; const float* src; int64 n; float one_minus_beta} records
 *      (locate_average_record_bytes() = 32, the float followed by 4 bytes of padding); chunks: DEVICE (tensor index, chunk index)
 *      int pairs in pieces of locate_average_chunk_elems().  Per element, three fp32 operations, each rounded once and never
 *      contracted: avg = avg + one_minus_beta * (src - avg).  A record whose one_minus_beta == 1.0f is copied bit for bit
 *      (avg = src, NaN and Inf payloads included).  avg and src need only 4-byte alignment (16-byte accesses are used where both
 *      are 16-byte aligned); they must not overlap.  Nothing outside [avg, avg + n) is written.  No allocation, host read or
 *      synchronisation: legal under stream capture. ---- */
size_t locate_average_record_bytes(void);
int locate_average_chunk_elems(void);
int locate_average_update(const void* tensors, const void* chunks, int n_tensors, int n_chunks, void* stream);

/* ---- per-tensor statistics with a non-finite guard (no reference counterpart), every tensor of a table in one pass over memory.
 *      tensors: DEVICE array of {const float* x; int64 n; int32 first_chunk; int32 pad} records
 *      (locate_stats_tensor_record_bytes() = 24); chunks: DEVICE (tensor index, chunk index) int pairs in pieces of
 *      locate_stats_chunk_elems(), a tensor's chunks consecutive and in ascending order, its chunk 0 at position first_chunk of
 *      the array.  records: n_tensors records {double sumsq; float absmax; uint32 nonfinite} (locate_stats_record_bytes() = 16),
 *      8-byte aligned:
 *        sumsq      sum of (double) x * (double) x over the FINITE elements (each square is exact; only the additions round:
 *                   within n 2^-52 relative of the exact sum);
 *        absmax     largest |x| among the finite elements, exact, denormals included; 0 if there is none;
 *        nonfinite  elements whose exponent field is all ones (NaN of either sign and any payload, +-Inf), modulo 2^32.
 *      summary: {uint32 total of nonfinite over the table; int32 index of the first tensor in table order that has one, or -1}.
 *      workspace: locate_stats_workspace_bytes(n_chunks) bytes, 8-byte aligned, need not be zeroed.
 *      A tensor's record depends only on its contents and n - not on the table around it, its position, its alignment (x needs
 *      4 bytes; 16-byte loads are used where a chunk is 16-byte aligned) or the grid: two calls give the same bits.  Two launches
 *      (a partial per chunk, then one block per tensor adds its partials in a fixed order); no floating-point atomics.  Only
 *      records, summary and workspace are written.  A table entry that is out of range or inconsistent is skipped: its record is
 *      then unspecified, and nothing outside the three outputs is written.  No allocation, host read or synchronisation: legal
 *      under stream capture.  At most locate_stats_max_blocks() blocks stride over the chunk table. ---- */
size_t locate_stats_tensor_record_bytes(void);
size_t locate_stats_record_bytes(void);
int locate_stats_chunk_elems(void);
int locate_stats_max_blocks(void);
size_t locate_stats_workspace_bytes(int n_chunks);
int locate_stats_reduce(const void* tensors, const void* chunks, int n_tensors, int n_chunks, void* records, void* summary,
                        void* workspace, void* stream);

/* ---- guarded Nadam step (no reference counterpart): locate_nadam_step behind a verdict taken on the device from the gradients.
 *      grads: DEVICE array of n_grads {const float* g; int64 n} records (locate_guard_tensor_record_bytes() = 16) over EVERY gradient
 *      of the optimizer, all parameter groups together; grad_chunks: DEVICE (tensor index, chunk index) int pairs in pieces of
 *      locate_guard_chunk_elems(); workspace: locate_guard_workspace_bytes(n_grad_chunks) bytes, 8-byte aligned, need not be zeroed.
 *      verdict: locate_guard_verdict_bytes() = 64 bytes, 8-byte aligned, zeroed ONCE by the caller, read and written:
 *        {double norm; uint64 nonfinite; float scale; int32 skip; int64 steps, skipped, clipped, consecutive_skips; double sumsq}
 *        sumsq      sum of (double) g * (double) g over the FINITE gradient elements (within n 2^-52 relative of the exact sum),
 *                   norm = sqrt(sumsq); nonfinite: elements whose exponent field is all ones;
 *        skip       skip_nonfinite != 0 && nonfinite > 0;
 *        scale      (float)(max_norm / norm), the division in double, when max_norm > 0 && norm > max_norm && !skip; else 1.0f
 *                   (torch's clip_grad_norm_ divides by norm + 1e-6 instead);
 *        steps counts the verdicts, skipped / clipped those with skip / a scale below 1, consecutive_skips the skipped steps since
 *        the last step that was taken.
 *      n_grads > 0: a reduce launch (at most locate_guard_max_blocks() blocks stride over the chunk table; 16-byte loads between a
 *      scalar head and tail, so g needs 4-byte alignment only) and a one-block verdict launch run first.  n_grads == 0 (then grads,
 *      grad_chunks, workspace NULL and n_grad_chunks 0): the verdict the record holds is applied - the later parameter groups of a step.
 *      Then, for the ONE parameter group given as in locate_nadam_step: skip == 0: the Nadam step on g * scale (one fp32 multiply,
 *      rounded on its own; weight decay added after it); scale == 1.0f gives locate_nadam_step's bits.  skip == 1: p, m, v, sched keep
 *      every bit; the absmax words are cleared and refilled with max |p|.  g is never written.  No floating-point atomics, no
 *      allocation, host read or synchronisation: legal under stream capture, where the decision is taken at every replay. ---- */
size_t locate_guard_tensor_record_bytes(void);
size_t locate_guard_verdict_bytes(void);
int locate_guard_chunk_elems(void);
int locate_guard_max_blocks(void);
size_t locate_guard_workspace_bytes(int n_chunks);
int locate_guarded_nadam_step(const void* grads, const void* grad_chunks, int n_grads, int n_grad_chunks, void* workspace, void* verdict,
                              double max_norm, int skip_nonfinite, const void* tensors, void* coef, const void* chunks, int n_tensors,
                              int n_chunks, double lr, double beta1, double beta2, double eps, double schedule_decay, double weight_decay,
                              void* stream);

/* ---- last-good copy of a training state in device memory (no reference counterpart): every tensor of a table into one of two
 *      slots in one pass that also classifies every 4-byte word it copies, and a one-block commit behind it.
 *      records: DEVICE array of {uint32* live; int64 offset; int64 n; int32 kind; uint32 fill[4]; int32 pad} records
 *      (locate_snapshot_record_bytes() = 48): live may be NULL (the tensor does not exist yet) and needs 4-byte alignment only;
 *      offset: BYTES into a slot, a multiple of 16; n: 4-byte words; kind: how a word is judged - 0 never, 1 fp32 (exponent field
 *      all ones), 2 fp64 (n even: the exponent field of the HIGH word of each pair all ones, the low word is not looked at).
 *      chunks: DEVICE (tensor index, chunk index) int pairs in pieces of locate_snapshot_chunk_elems() words.
 *      slot0, slot1: 16-byte aligned, distinct, each at least max(offset + 4 n) bytes.
 *      commit: locate_snapshot_commit_bytes() = 64 bytes, 8-byte aligned, read and written:
 *        {int32 good; int32 bad_tensor; uint64 bad_words; int64 iteration, taken, rejected, last_rejected_iteration,
 *         last_rejected_count; int32 last_rejected_tensor; int32 pad}
 *        set ONCE by the caller to good = -1, bad_tensor = INT32_MAX, last_rejected_tensor = -1, everything else 0.
 *      locate_snapshot_take, two launches: (1) copies every tensor bit for bit (NaN payloads, denormals, -0.0) to its offset in
 *      the slot that is not `good` (slot0 when good == -1) - for a NULL live pointer the four fill words, repeating - and counts
 *      the words that are non-finite for their kind: blocks that found one add their count to bad_words and fold the lowest such
 *      tensor index into bad_tensor (one integer atomic each per block; no floating-point atomics; a clean take issues none);
 *      (2) one block: bad_words == 0: good = the slot just written, iteration = `iteration`, taken += 1; otherwise good and
 *      iteration stay, rejected += 1, last_rejected_{iteration, count, tensor} are stored.  bad_words and bad_tensor are reset:
 *      the record is ready for the next take.  16-byte accesses where live is 16-byte aligned; every load of a chunk is issued
 *      before its first store.  Writes the destination slot and the commit record and nothing else; the live tensors and the
 *      good slot are only read.  No allocation, host read or synchronisation: legal under stream capture, where the decision
 *      is taken at every replay.
 *      locate_snapshot_restore: `slot` (the caller chooses: slot `good`) back into the live tensors; writes exactly
 *      [live, live + n) of every record whose live pointer is not NULL. ---- */
size_t locate_snapshot_record_bytes(void);
size_t locate_snapshot_commit_bytes(void);
int locate_snapshot_chunk_elems(void);
int locate_snapshot_take(const void* records, const void* chunks, int n_tensors, int n_chunks, void* slot0, void* slot1, void* commit,
                         long long iteration, void* stream);
int locate_snapshot_restore(const void* records, const void* chunks, int n_tensors, int n_chunks, const void* slot, void* stream);

/* ---- 128-bit digests of every tensor of a device table, over 4-byte words, modulo 2^64 (no reference counterpart; what the
 *      snapshot's spill to disk checks a copy against, locate_amd/spill.py):  A = sum_i w_i,  B = sum_i ((i + 1) mod 2^32) * w_i.
 *      records: DEVICE array of {const uint32* p; int64 n} records (locate_digest_record_bytes() = 16); p needs 4-byte alignment
 *      only; n may be 0.  chunks: DEVICE (tensor index, chunk index) int pairs in pieces of locate_digest_chunk_elems() words, a
 *      tensor's pairs consecutive and in order.  first: DEVICE int32[n_tensors + 1], the position of each tensor's first pair,
 *      n_chunks at the end.  partials: n_chunks x 16 bytes, out: n_tensors x {uint64 A, uint64 B}, both 8-byte aligned.
 *      Two launches: one {A, B} partial per pair (a damaged pair writes zeros), then each tensor's partials over
 *      [first[t], first[t + 1]) added into out[t].  Integer sums only, no atomics, nothing to clear between calls: the result
 *      depends on nothing but the words and their order.  No allocation, host read or synchronisation: legal under stream
 *      capture.  Only partials and out are written. ---- */
size_t locate_digest_record_bytes(void);
int locate_digest_chunk_elems(void);
int locate_digest(const void* records, const void* chunks, const void* first, int n_tensors, int n_chunks, void* partials, void* out,
                  void* stream);

/* ---- per-tensor deltas against a base copy (no reference counterpart; locate_amd/dynamics.py), every tensor of a table in one
 *      pass over memory.  tensors: DEVICE array of {const float* w; float* base; int64 n; int32 first_chunk; int32 pad} records
 *      (locate_dyn_tensor_record_bytes() = 32): w the live tensor, base its n-element slot in an arena the caller owns; chunks:
 *      DEVICE (tensor index, chunk index) int pairs in pieces of locate_dyn_chunk_elems(), a tensor's chunks consecutive and in
 *      ascending order, its chunk 0 at position first_chunk of the array.  With d[i] = w[i] - base[i] (one fp32 subtraction,
 *      denormals kept), records: n_tensors records (locate_dyn_record_bytes() = 32), 8-byte aligned:
 *        double delta_sumsq   sum of (double) d * (double) d over the FINITE d (exact squares; within n * 2^-52 relative)
 *        double base_sumsq    the same sum over the finite base[i]
 *        uint32 delta_absmax  bit pattern of the largest finite |d|, 0 if there is none
 *        uint32 unchanged     elements with w[i] == base[i] compared as fp32 (+0 == -0 counts, a NaN never does), modulo 2^32
 *        uint32 nonfinite     elements whose d is NaN or +-Inf (left out of the two delta fields), modulo 2^32
 *        uint32 pad           0
 *      mode 1 (record): writes records and workspace, only reads base.  mode 2 (rebase): base[i] = w[i] bit for bit, NaN
 *      payloads included; no record: records and workspace may be NULL.  mode 3: both in one pass; the records describe the base
 *      as it was.  workspace: locate_dyn_workspace_bytes(n_chunks) bytes, 8-byte aligned, need not be zeroed.
 *      A tensor's record depends only on its contents and n - not on the table around it, its position, the alignment of w or
 *      base (4 bytes are enough; 16-byte loads and stores are used where a chunk of both is 16-byte aligned) or the grid: two
 *      calls give the same bits.  No floating-point atomics.  A table entry that is out of range or inconsistent is skipped:
 *      its record is then unspecified, and nothing is written through it.  One launch (rebase) or two; no allocation, host
 *      read or synchronisation: legal under stream capture.  At most locate_dyn_max_blocks() blocks stride over the chunk
 *      table. ---- */
size_t locate_dyn_tensor_record_bytes(void);
size_t locate_dyn_record_bytes(void);
int locate_dyn_chunk_elems(void);
int locate_dyn_max_blocks(void);
size_t locate_dyn_workspace_bytes(int n_chunks);
int locate_dyn_pass(const void* tensors, const void* chunks, int n_tensors, int n_chunks, int mode, void* records, void* workspace,
                    void* stream);

/* ---- what a reduced-precision format would do to a contraction operand (no reference counterpart; locate_amd/formats.py).
 *      host_views: HOST array of n_views (1 .. locate_formats_max_views() = 8) records {const float* x; int32 B, C, P; int64
 *      batch_stride; int32 axis} (natural C layout, locate_formats_view_record_bytes() = 40): element (b, c, p) at
 *      x[b * batch_stride + c * P + p]; the 32-element scale blocks run along c (axis 1: 32 consecutive c at fixed (b, p)) or
 *      along p (axis 2: 32 consecutive p at fixed (b, c)), a line's last block covers the members that exist.  x: DEVICE fp32,
 *      4-byte aligned; fewer than 2^31 elements.  The records travel by value in the launch arguments: no device table.
 *      rows: DEVICE slots of locate_formats_base_record_bytes() + locate_formats_count() * locate_formats_format_record_bytes()
 *      = 304 + 5 * 32 = 464 bytes, 8-byte aligned; view i ADDS into slot row_slots[i] (HOST array; no two views of a call share
 *      a slot; the caller zeroes a slot before its first call):
 *        base    uint64 n           elements
 *                uint64 zeros       +-0 elements
 *                uint64 nonfinite   NaN and +-Inf elements: counted here and left out of everything else
 *                uint64 calls       calls added into this slot
 *                double sumsq       sum of (double) x * (double) x over the finite elements (exact squares)
 *                uint32 absmax      bit pattern of the largest finite magnitude (over calls: the maximum); uint32 pad
 *                uint64 hist[32]    finite non-zero elements by fp32 exponent field (0 counted as 1): bin j lies j below the
 *                                   field of THIS CALL's absmax, bin 31 takes everything lower
 *        format  double err_sumsq   sum of e * e, e = (double) x - (double) q * 2^-scale in double (exact squares)
 *                uint64 flushed     x finite and non-zero, q == 0
 *                uint64 subnormal   q != 0 and |q| below the grid's smallest normal
 *                uint64 clamped     the rounded magnitude exceeded the grid's maximum (q is then the maximum)
 *      Formats (locate_formats_name(i)), every one rounded to nearest even onto its grid, subnormals included:
 *        0 e4m3_tensor  3 mantissa bits, smallest normal 2^-6, max 448; one 2^k per tensor, absmax * 2^k in [2^7, 2^8) (the
 *                       rule of the fp8 contractions); v_cvt_pk_fp8_f32 / v_cvt_f32_fp8
 *        1 e5m2_tensor  2, 2^-14, 57344; one 2^k per tensor, absmax * 2^k in [2^14, 2^15); v_cvt_pk_bf8_f32 / v_cvt_f32_bf8
 *        2 mxfp8_e4m3   grid of 0; per scale block 2^X, X = clamp(max(field(A), 1) - 127 - 8, -127, 127), A the block's largest
 *                       finite magnitude (OCP MX v1.0)
 *        3 mxfp4_e2m1   1, 2^0, 6; the same with - 2
 *        4 bf16         7, 2^-126, largest finite bf16; no scale
 *      workspace: DEVICE, locate_formats_workspace_bytes(host_views, n_views) bytes (0 for damaged views), 8-byte aligned, need
 *      not be zeroed.  A view's contribution depends only on its contents and (B, C, P, axis) - not on alignment, batch_stride,
 *      the other views or the grid: two calls give the same bits.  Four launches (a grid pass and a one-block-per-view sum,
 *      twice: the per-tensor scales need absmax first, which the second pass reads from the workspace); no floating-point
 *      atomics, no allocation, host read or synchronisation: legal under stream capture.  Damaged arguments (n_views out of
 *      range, axis not 1 or 2, a non-positive extent, batch_stride below C * P, a misaligned or null address, a shared or
 *      negative slot) return an error status and launch nothing. ---- */
int locate_formats_count(void);
const char* locate_formats_name(int i);          /* NULL outside [0, locate_formats_count()) */
int locate_formats_max_views(void);
size_t locate_formats_view_record_bytes(void);
size_t locate_formats_base_record_bytes(void);
size_t locate_formats_format_record_bytes(void);
size_t locate_formats_workspace_bytes(const void* host_views, int n_views);
int locate_formats_audit(const void* host_views, int n_views, const int* row_slots, void* rows, void* workspace, void* stream);

/* ---- loss glue (main.py:149-156,164-169, libs/utils.py:133-134, libs/grad_penalty.py:1-2): values and the
 *      gradients w.r.t. the discriminator outputs ---- */
int locate_d_loss(const float* d_true, const float* d_fake, const float* d_aug, int B, float gamma, float* losses,
                  float* g_true, float* g_fake, float* g_aug, void* stream);
int locate_g_loss(const float* d_fake, int B, float* loss, float* g_fake, void* stream);

/* ---- device-side input pipeline (libs/utils.py:88-113: the reference's two ImageFolder transform chains, which it runs on the
 *      CPU with torchvision / PIL).  `store`: uint8 [N, H, W, 3] device memory, 16-byte aligned - the data set after the
 *      deterministic decode + Resize(2 S).  One call makes n samples: sample i reads image idx[i] and applies record i of `params`
 *      (locate_input_param_record_bytes() = 32 bytes: int32 flip; int32 order - four 4-bit op codes, first op in the low bits,
 *      0 brightness, 1 contrast, 2 saturation, anything else no-op (hue is off in the reference), so 0x3333 is the plain chain;
 *      float brightness, contrast, saturation factors; int32 top, left, side of the square crop of the flipped image), then
 *      resizes the crop to S x S and writes (u8 / 255 - 0.5) / 0.5 as fp32 [3, S, S]: samples [0, n_first) into out_first, the
 *      others into out_rest (the plain and the augmented batch of one step in one launch).  The arithmetic is Pillow's, bit for
 *      bit: Image.blend in fp32 per jitter op with uint8 between the ops, the contrast mean over the whole source image, the
 *      antialiased BILINEAR resize in 22-bit fixed point, horizontal pass first.
 *      `coef`: int32 [side_hi - side_lo + 1][S][2 + ktaps] = {first tap, tap count, weights * 2^22} per crop side and output
 *      index (one table serves both axes); `lut`: the 256 output values; both built by the caller (locate_amd/data.py) so that
 *      nothing depends on how the device rounds.  `workspace`: locate_input_workspace_bytes(n, H, W) bytes, need not be zeroed.
 *      The caller guarantees idx[i] < N and crops inside the image with side in [side_lo, side_hi]; a record that breaks this
 *      leaves its output untouched. ---- */
size_t locate_input_param_record_bytes(void);
int locate_input_mean_blocks(int H, int W);      /* blocks per sample of the contrast pass = int32 words of workspace per sample */
size_t locate_input_workspace_bytes(int n, int H, int W);
int locate_input_transform(const void* store, int N, int H, int W, const int32_t* idx, const void* params, int n, int n_first,
                           const int32_t* coef, int side_lo, int side_hi, int ktaps, const float* lut, int S, float* out_first,
                           float* out_rest, void* workspace, void* stream);

/* ---- training monitor (main.py:194-225: the reference's sample picture, which it makes on the host with torchvision's
 *      make_grid(padding, normalize=True) and matplotlib's imsave).  x: fp32 [n, 3, S, S], contiguous, device memory.
 *      locate_image_range: range = {min(x), max(x)} over all n_elems values (both NaN if x holds a NaN); exact in any order, no
 *      atomics on values.  `workspace`: locate_image_range_workspace_bytes() bytes, need not be zeroed.
 *      locate_image_grid: the tiled picture.  xmaps = min(nrow, n), ymaps = ceil(n / xmaps), GH = (S + padding) ymaps + padding,
 *      GW = (S + padding) xmaps + padding; image k at row (k / xmaps)(S + padding) + padding, column (k % xmaps)(S + padding) +
 *      padding; every other pixel is pad_value (not normalised; meant to lie in [0, 1]).  Per value, in fp32 IEEE operations:
 *      v = (min(max(x, lo), hi) - lo) / d with d = (float) max((double) hi - (double) lo, 1e-5) when `divisor` is 0, else d =
 *      divisor (a caller-supplied range: the caller takes hi - lo from its own doubles); byte = (uint8) (v * 255.0f), truncated.
 *      grid_f32 [3, GH, GW] (what make_grid returns) and grid_u8 [GH, GW, 4] (RGBA, alpha 255: what imsave encodes): either may
 *      be null, not both.  `range` is device memory {lo, hi}: locate_image_range's output or the caller's bounds.  A non-finite
 *      x gives unspecified bytes. ---- */
size_t locate_image_range_workspace_bytes(void);
int locate_image_range(const float* x, int64_t n_elems, float* range, void* workspace, void* stream);
int locate_image_grid(const float* x, int n, int S, int nrow, int padding, float pad_value, const float* range, float divisor,
                      float* grid_f32, uint8_t* grid_u8, void* stream);

/* ---- sliced Wasserstein distance between Laplacian-pyramid patch descriptors (Karras et al., "Progressive Growing of GANs",
 *      section 5; the reference has no quality metric).  Every call is stateless, uses no atomics and returns the same bits from
 *      call to call.  All tensors fp32, contiguous, device memory.
 *      Pyramid: g = outer([1,4,6,4,1], [1,4,6,4,1]) / 256, borders mirrored without repeating the edge sample (-1 -> 1, -2 -> 2,
 *      H -> H - 2, H + 1 -> H - 3).  pyr_down: x [planes, S, S] -> out [planes, S/2, S/2], out[i, j] = sum_ab g[a, b]
 *      x[m(2i + a - 2), m(2j + b - 2)]; S even, >= 8.  pyr_residual: out = x - up(coarse), coarse [planes, S/2, S/2], up = coarse
 *      written into the even positions of a zero map of size S and filtered with 4 g (mirror on that doubled grid); evaluated in
 *      its polyphase form, the upsampled map is never stored; out may be x.
 *      Descriptors: descriptor j of n = N P belongs to image j / P; pos int32 [n, 2] = (y, x) of its top-left corner in
 *      [0, S - 7] (a record outside is clamped into it); element k = c 49 + dy 7 + dx is level[j / P, c, y + dy, x + dx], K = 147.
 *      swd_stats: stats[6] = {mu_0, mu_1, mu_2, r_0, r_1, r_2}: per channel the mean and 1 / the population deviation over all
 *      n 49 gathered values (patches overlap: not the statistic of the map), fp64 sums in a fixed order, each rounded once to fp32.
 *      A constant channel gives a non-finite r; it is not guarded.  `workspace`: locate_swd_stats_workspace_bytes() bytes, 8-byte
 *      aligned, need not be zeroed.
 *      swd_project: proj [D, n] (direction-major), proj[d, j] = sum_k dirs[k, d] ((v_jk - mu_c(k)) r_c(k)), dirs [147, D]; the
 *      mean is subtracted from the gathered value before the multiplication, the sum is a k-ordered fp32 fmaf chain
 *      (v_mfma_f32_32x32x2_f32).  N 3 S S and N P below 2^31.
 *      swd_distance: out[0] = mean_i |a[i] - b[i]| over `count` values (two sorted projection sets; the sort is the caller's):
 *      the difference in fp32, the sum in fp64 in a fixed order, one rounding to fp32.  `workspace`:
 *      locate_swd_distance_workspace_bytes() bytes, 8-byte aligned. ---- */
int locate_pyr_down(const float* x, int planes, int S, float* out, void* stream);
int locate_pyr_residual(const float* x, const float* coarse, int planes, int S, float* out, void* stream);
size_t locate_swd_stats_workspace_bytes(void);
int locate_swd_stats(const float* level, int N, int S, const int32_t* pos, int P, float* stats, void* workspace, void* stream);
int locate_swd_project(const float* level, int N, int S, const int32_t* pos, int P, const float* dirs, int D, const float* stats,
                       float* proj, void* stream);
size_t locate_swd_distance_workspace_bytes(void);
int locate_swd_distance(const float* a, const float* b, int64_t count, float* out, void* workspace, void* stream);

/* ---- exact nearest neighbours in the 8-bit domain (csrc/neighbours.hip; locate_amd/neighbours.py).  Integers throughout: the
 *      result depends on nothing but the bytes, no atomics.
 *      Code of an image x fp32 [3, S, S], per element: t = fmul_rn(fadd_rn(x, 1), 127.5); u = 0 for t < 0, 255 for t > 255, else
 *      rintf(t) (ties to even); code = u - 128 as int8.  A row holds the codes in c, y, x order in row_bytes = roundup(3 S^2, 64)
 *      bytes (locate_nn_row_bytes; 0 for S outside 1 .. 4096), the pad bytes 0.  norms[i] = int64 sum of code^2; nonfinite[i] = the
 *      number of NaN / Inf elements (their code byte is 0; an image with any is "flagged").  x 4-byte aligned (16-byte loads when it
 *      is 16-byte aligned and 3 S^2 a multiple of 4), codes 16-byte aligned.
 *      locate_nn_search: d2(q, r) = sum (code_q - code_r)^2 = norm_q + norm_r - 2 dot(q, r), the dot product on
 *      v_mfma_i32_32x32x32_i8, rows longer than 65536 bytes in int32 segments added in int64.  Per query the k (1 .. 8) references
 *      with the smallest (d2, index) in lexicographic order into d2 int64 [Q, k] / index int32 [Q, k]; empty slots (fewer than k
 *      candidates) hold -1 / -1, as does every slot of a flagged query (qflags[i] != 0).  A reference with rflags[j] != 0 (rflags
 *      may be null: none) is never returned, nor is reference skip[i] for query i (skip may be null; -1: none).  qcodes [Q, row_bytes],
 *      rcodes [N, row_bytes], 16-byte aligned; row_bytes a multiple of 64, at most 262144; N < 2^30.  The norms must be those of the
 *      rows.  `workspace`: locate_nn_search_workspace_bytes(Q, N, k) bytes, 8-byte aligned, need not be zeroed. ---- */
int locate_nn_row_bytes(int S);
int locate_nn_encode(const float* x, int n, int S, int8_t* codes, int64_t* norms, int32_t* nonfinite, void* stream);
size_t locate_nn_search_workspace_bytes(int Q, int N, int k);
int locate_nn_search(const int8_t* qcodes, const int64_t* qnorms, const int32_t* qflags, int Q, const int8_t* rcodes, const int64_t* rnorms,
                     const int32_t* rflags, int N, int row_bytes, const int32_t* skip, int k, int64_t* d2, int32_t* index, void* workspace,
                     void* stream);

/* ---- "which balls is each query in": the counts behind precision / recall / density / coverage (csrc/neighbours.hip;
 *      locate_amd/manifold.py).  The conventions, the distances and the limits of locate_nn_search.  The pair (q, r) counts iff
 *      qflags[q] == 0, rflags[r] == 0 (rflags may be null: none flagged), radius2[r] >= 0 (a negative radius: this reference has no
 *      ball), r != skip[q] (skip may be null; -1: none) and d2(q, r) <= radius2[r], compared in int64.  hits int32 [Q]: the counting
 *      pairs of each query; covered int32 [N]: those of each reference - may be null: then no work and no workspace for it.  Two
 *      launches, no atomics: every block writes its counts, a second kernel adds them in ascending tile order; two calls give the
 *      same words.  radius2 int64 [N], 8-byte aligned.  `workspace`: locate_nn_within_workspace_bytes(Q, N, covered != null) bytes,
 *      4-byte aligned; neither it nor the outputs need be zeroed. ---- */
size_t locate_nn_within_workspace_bytes(int Q, int N, int want_covered);
int locate_nn_within(const int8_t* qcodes, const int64_t* qnorms, const int32_t* qflags, int Q, const int8_t* rcodes, const int64_t* rnorms,
                     const int32_t* rflags, int N, int row_bytes, const int64_t* radius2, const int32_t* skip, int32_t* hits, int32_t* covered,
                     void* workspace, void* stream);

/* ---- sums of groups of code rows and their rounded means: the centroid update of an exact k-means in the 8-bit domain
 *      (csrc/modes.hip; locate_amd/modes.py; the definition in int64 numpy: tests/helpers/modes_model.py).  Integers throughout.
 *      locate_nn_group_sums: codes int8 [N, row_bytes] as locate_nn_encode writes them, 16-byte aligned, row_bytes a multiple of
 *      64, at most 262144, N >= 1.  order int32 [M]: image indices, not necessarily distinct; an index outside 0 .. N - 1
 *      contributes nothing.  starts int32 [K + 1]: group k is order[lo_k : hi_k] with lo_k = clamp(starts[k], 0, M) and hi_k =
 *      clamp(starts[k + 1], 0, M), empty when hi_k <= lo_k.  starts[0] need not be 0 (what precedes it belongs to no group),
 *      `starts` need not increase (groups may then overlap; each is summed as defined), and no value of `order` or `starts` makes
 *      a kernel read outside codes, order or starts.  sums int32 [K, row_bytes]: sums[k][j] = the sum of codes[i][j] over group
 *      k, a row of zeros for an empty group; every word is written.  1 <= M <= 2^24 - 1 (|sum| <= 128 M < 2^31: exact) and
 *      1 <= K <= 65535, anything else is refused before a launch.  Two launches, no atomics: a walk over slabs of 64 positions of
 *      `order` that reads every row once and stores a partial sum wherever a group begins or ends, then per group the sum of its
 *      partials; two calls give the same words.  `workspace`: locate_nn_group_sums_workspace_bytes(M, K, row_bytes) =
 *      4 (slots (row_bytes + 1) + 2 (K + 1)) bytes with slots = ceil(M / 64) + K + 1 (0 for sizes that are refused), 16-byte
 *      aligned; neither it nor sums need be zeroed.  order, starts, sums 4-byte aligned.
 *      locate_nn_centroids: with n = hi_k - lo_k from `starts` and M as above, row k of codes int8 [K, row_bytes] is, per byte,
 *      floor((2 sums[k][j] + n) / (2 n)) - FLOOR division, a half goes towards +infinity - for n > 0, which lies in -128 .. 127
 *      when sums are those of n codes (pad bytes: 0), and row k of `previous` byte for byte for n = 0.  `previous` may be `codes`:
 *      every byte is read before it is written.  norms int64 [K]: the sum of the squares of the row written; moved int32 [K]: the
 *      bytes of row k that differ from previous[k] (0 for an empty group).  One launch, a block per row, no atomics.  sums,
 *      previous and codes 16-byte, norms 8-byte, starts and moved 4-byte aligned; the limits on M, K and row_bytes as above. ---- */
size_t locate_nn_group_sums_workspace_bytes(int M, int K, int row_bytes);
int locate_nn_group_sums(const int8_t* codes, int N, int row_bytes, const int32_t* order, int M, const int32_t* starts, int K,
                         int32_t* sums, void* workspace, void* stream);
int locate_nn_centroids(const int32_t* sums, const int32_t* starts, int K, int M, int row_bytes, const int8_t* previous,
                        int8_t* codes, int64_t* norms, int32_t* moved, void* stream);

/* ---- radial power spectrum of image planes (csrc/spectrum.hip; locate_amd/spectrum.py).  Per plane x fp32 [S, S], S in {32, 64,
 *      128, 256}, H = S / 2, against the caller's tables cos_table / sin_table fp32 [S][S] (C[k][j] = cos(2 pi k j / S) w[j], Sn
 *      likewise; 16-byte aligned): Ar[y][k] = sum_x x[y][x] C[k][x], Ai[y][k] = - sum_x x[y][x] Sn[k][x]; Yr[a][k] = sum_y C[a][y]
 *      Ar[y][k] + Sn[a][y] Ai[y][k], Yi[a][k] = sum_y C[a][y] Ai[y][k] - Sn[a][y] Ar[y][k] for a = 0 .. S - 1, k = 0 .. H, every sum
 *      in fp32 on v_mfma_f32_16x16x4_f32 (the summation order is the kernel's own); power[a][k] = ((double) Yr^2 + (double) Yi^2)
 *      m[k] / S^4, m = 1 for k in {0, H} and 2 otherwise.  The radial bins arrive sorted: slot int32 [S][H + 1] is the place of
 *      (a, k) in the list of all S (H + 1) frequencies ordered by (bin, a, k), start int32 [R + 1] the bins' first places
 *      (start[R] = S (H + 1)); entries outside the list are clamped into it.  spectra float64 [planes][R]: spectra[p][r] = the sum
 *      of the powers of bin r, four interleaved partial sums added as (p0 + p1) + (p2 + p3).  No atomics: the same words from call
 *      to call, whatever else is in the call and whatever the alignment of x (4-byte; S >= 128: 16-byte).  A plane that holds a
 *      NaN or an Inf gives a spectrum that is not finite.  S <= 64 is one launch and needs no workspace (it may be null); S >= 128
 *      is three launches through `workspace`: locate_spectrum_workspace_bytes(planes, S) bytes, 16-byte aligned, need not be zeroed.
 *      locate_spectrum_summary: spectra float64 [n][channels][R], count float64 [R] (a bin's multiplicity).  flags (`workspace`:
 *      locate_spectrum_summary_workspace_bytes(n channels) bytes, 4-byte aligned) mark the planes whose spectrum is not finite; then
 *      per (channel, bin), over the OTHER planes of the channel in ascending order (one fixed block sum): sums[0][c][r] = sum of
 *      spectra / count, sums[1][c][r] = sum of its square (sums float64 [2][channels][R]); nonfinite int32 [channels] = the marked
 *      planes of each channel.  Two launches, no atomics. ---- */
size_t locate_spectrum_workspace_bytes(int planes, int S);
int locate_spectrum_planes(const float* x, int planes, int S, const float* cos_table, const float* sin_table, const int32_t* slot,
                           const int32_t* start, int R, double* spectra, void* workspace, void* stream);
size_t locate_spectrum_summary_workspace_bytes(int planes);
int locate_spectrum_summary(const double* spectra, int n, int channels, int R, const double* count, double* sums, int32_t* nonfinite,
                            void* workspace, void* stream);

/* ---- multi-scale SSIM of image pairs in the 8-bit domain (csrc/msssim.hip; locate_amd/msssim.py; the definition in float64 numpy:
 *      tests/helpers/msssim_model.py).  Pair i is row i of `a` against row i of `b`: code rows as locate_nn_encode writes them (c, y, x
 *      order, value = code + 128), 16-byte aligned, row_bytes >= 3 S^2 a multiple of 16; S in {32, 64, 128, 256}.  Five levels of side
 *      S >> l, level l + 1 the 2 x 2 mean of level l (exact in fp32); per level the n = min(11, side) taps of row l of `taps` (float64
 *      [5][11], zero padded), "valid", rows then columns, every product and sum in float64 in one fixed order.  out float64
 *      [pairs][2][5]: the means over the three channels' outputs of ssim (out[i][0][l]) and cs (out[i][1][l]).  The flags (int32
 *      [pairs], locate_nn_encode's) may be null; a pair with a flagged member gets ten NaNs.  No atomics: a pair's ten numbers depend
 *      on its two rows alone, (a, b) gives the bits of (b, a), and a row against itself 1.0 ten times.  S <= 64 is one launch and needs
 *      no workspace (it may be null); 128 is two launches, 256 three, through `workspace`: locate_msssim_workspace_bytes(pairs, S)
 *      bytes, 16-byte aligned, need not be zeroed, and at most 65535 pairs a call. ---- */
size_t locate_msssim_workspace_bytes(int pairs, int S);
int locate_msssim_pairs(const int8_t* a, const int32_t* aflags, const int8_t* b, const int32_t* bflags, int pairs, int row_bytes, int S,
                        const double* taps, double* out, void* workspace, void* stream);

/* ---- differentiable augmentation of an image batch and its adjoint (csrc/diffaug.hip; locate_amd/augment.py; the definition in
 *      float64 numpy: tests/helpers/diffaug_model.py).  x, y fp32 [n, 3, S, S] contiguous, 4-byte aligned (16-byte stores and loads
 *      where a buffer allows them; the values do not depend on it), S in {32, 64, 128, 256}, n <= 65535; params fp32 [n, 12], one row
 *      per image: b, s, c, ty, tx, y0, y1, x0, x1, mask, 0, 0 (the integers exact in fp32; mask 0: every op of the policy runs - below).  policy: bit 0 colour, bit 1 translation,
 *      bit 2 cutout - it selects the kernel, and an op that is off reads none of its words and executes none of its arithmetic.
 *      Forward: z = c (s (x - mu) + mu - M) + M + b with mu the mean over the three channels of a pixel and M the image's mean; w the
 *      gather z[c, i - ty, j - tx], exactly 0.0 outside the frame; y = keep * w, keep = 0.0f on [y0, y1) x [x0, x1) and 1.0f elsewhere,
 *      an fp32 multiplication.  Backward: gz[c, p] = keep[p + t] gy[c, p + t] inside the frame, else 0; gx = c s gz + c (1 - s)
 *      mean_c gz + (1 - c) mean(gz).  M and mean(gz) are float64 sums in one fixed order, divided by 3 S^2 and rounded once to fp32;
 *      no atomics: an image's result depends on that image and its row alone.  S <= 64 is one launch and needs no workspace (it may
 *      be null); S >= 128 with colour is two launches through `workspace`: the workspace-bytes call's count, 8-byte aligned, need not
 *      be zeroed.  No allocation, no host read: legal under stream capture. ---- */
int locate_diffaug_param_floats(void);
size_t locate_diffaug_workspace_bytes(int n, int S);
int locate_diffaug_fwd(const float* x, const float* params, float* y, int n, int S, int policy, void* workspace, void* stream);
int locate_diffaug_bwd(const float* gy, const float* params, float* gx, int n, int S, int policy, void* workspace, void* stream);

/* ---- adaptive augmentation beside the training step (csrc/ada.hip; locate_amd/augment.py, AdaptiveDiffAugment; the definition in
 *      numpy, which both entries equal with ==: tests/helpers/ada_model.py).  Word 9 of a diffaug parameter row is a per-image op
 *      mask, a small exact integer in fp32: bit k set switches op k off for that image, and the image's result is then, bit for bit,
 *      that of the policy without those bits.  state: a record of 16 32-bit words at a fixed device address - 0 p (fp32), 1 r of the
 *      last closed window (fp32), 2 window sum, 3 logits counted in the window, 4 observations in the window, 5 windows closed, 6 ups,
 *      7 downs, 8 NaN logits seen, 9 ring rows written, 10 .. 15 zero.
 *      gate: raw_rows fp32 [n, 12] hold words 0 .. 8 of a row and, in words 9 .. 11, a uniform g_k in [0, 1) per op; out_rows gets
 *      words 0 .. 8 bit for bit, the mask in word 9 (bit k set where op k is in `policy` and not g_k < p, p = state word 0) and zeros.
 *      observe: adds #(x > 0) - #(x < 0) and the count of the non-NaN ones of the B logits to the window; the interval-th
 *      observation closes it: r = (float)((double)sum / (double)counted), p = min(max(p +- step, 0), p_max) for r > / < target (one
 *      fp32 addition), {iteration, r, p, counted} into ring row (rows written) % capacity (4 words a row).  One block, integer sums:
 *      order-free.  No allocation, no host read, no atomics: legal under stream capture. ---- */
int locate_ada_gate(const float* raw_rows, const void* state, float* out_rows, int n, int policy, void* stream);
int locate_ada_observe(const float* d_true, int B, int iteration, void* state, void* ring, int capacity, int interval, float target, float step,
                       float p_max, void* stream);

/* ---- LeCam regularisation of the discriminator (csrc/lecam.hip; locate_amd/lecam.py, LeCam; the definition in numpy, which both
 *      entries equal with ==: tests/helpers/lecam_model.py).  state: a record of 16 32-bit words at a fixed device address - 0 alpha_R,
 *      the anchor of mean D(real) (fp32), 1 alpha_F, the anchor of mean D(G(z)) (fp32), 2 observations accepted, 3 observations in
 *      all, 4 observations refused as non-finite, 5 ring rows written, 6 and 7 the last observation's two means (fp32), 8 .. 15 zero.
 *      d_loss_lecam: the arguments of locate_d_loss plus the record (read only); losses holds 4 floats {d_error, penalty, total, R}.
 *      Active iff weight != 0 and word 2 >= max(warmup, 1): total = (d_error + penalty) + weight * R with R = mean (t - alpha_F)^2
 *      + mean (alpha_R - f)^2 (one_sided != 0: both differences through clamp(min=0) first), and the gradients of it.  Inactive:
 *      losses[0 .. 3) and the three gradients are locate_d_loss's bits and R = 0.
 *      observe: d_gen is MINUS D(G(z)), the training step's out["d_gen"]; rate = fp32(1 - decay), in [0, 1].  The batch means in
 *      float64; both finite: the first accepted observation sets the anchors, later ones do alpha += rate * (m - alpha) (three fp32
 *      operations); otherwise the anchors stay and word 4 counts one.  {iteration, alpha_R, alpha_F, m_R, m_F, accepted, 0, 0} goes
 *      into ring row (rows written) % capacity (8 words a row).  One block each, no allocation, no host read, no atomics: legal
 *      under stream capture. ---- */
int locate_d_loss_lecam(const float* d_true, const float* d_fake, const float* d_aug, int B, float gamma, const void* state, float weight,
                        int one_sided, int warmup, float* losses, float* g_true, float* g_fake, float* g_aug, void* stream);
int locate_lecam_observe(const float* d_true, const float* d_gen, int B, int iteration, void* state, void* ring, int capacity, float rate,
                         void* stream);

/* ---- Top-k training of the generator (csrc/topk.hip; locate_amd/topk.py, TopK; the definition in numpy, which the entry equals
 *      with ==: tests/helpers/topk_model.py).  locate_g_loss's launch in which only the k logits that stand first contribute to
 *      losses[0] and to g_fake.  j stands before i iff f_j is a NaN and f_i is not, or both are and j < i, or neither is and f_j > f_i,
 *      or neither is, f_j == f_i (-0 == +0) and j < i; an element is kept iff fewer than k_used stand before it.  record: 16 32-bit
 *      words at a fixed device address - 0 k (int32, read only; outside 1 .. B: k_used = B), 1 launches, 2 launches whose logits held
 *      a NaN or an Inf, 3 k_used, 4 kept elements with (1 - f) >= 0, 5 the fp32 bits of the kept element of rank k_used - 1, 6
 *      (float)(sum f / B), 7 (float)(sum_kept f / k_used), 8 .. 15 zero.  ring: `capacity` rows of 8 words {launch ordinal (1-based),
 *      k_used, active, threshold, mean_all, mean_kept, non-finite 0 / 1, 0}, row (ordinal - 1) % capacity.  losses: 2 floats
 *      {loss_topk = (float)(sum_kept relu(1 - f) / k_used), loss_all = locate_g_loss's bits}; g_fake[i] = -(1 / k_used) where i is
 *      kept and (1 - f_i) >= 0, else +0.  1 <= B <= 4096.  form: 0 chooses the selection by B, 1 counts ranks, 2 sorts; the same bits.
 *      One block, no allocation, no host read, no atomics: legal under stream capture. ---- */
int locate_g_loss_topk(const float* d_fake, int B, void* record, void* ring, int capacity, int form, float* losses, float* g_fake,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
