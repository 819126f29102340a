// extern "C" surface of libsoccdpt_hip.so (see include/soccdpt_hip.h).
#include <hip/hip_runtime.h>

#include <cstring>
#include <cstdlib>
#include <string>

#include "internal.h"
#include "calibrate.h"
#include "train.h"
#include "kernels.h"
#include "occ_eval.h"
#include "visualise.h"
#include "occ_rays.h"
#include "occ_view.h"
#include "batch_targets.h"
#include "../../include/soccdpt_vis.h"
#include "../../include/soccdpt_occ_rays.h"
#include "../../include/soccdpt_occ_view.h"
#include "../../include/soccdpt_data.h"

using namespace soccdpt;

static std::string g_create_error;

namespace soccdpt {
LaunchTimer*& launch_timer() {
    static thread_local LaunchTimer* t = nullptr;
    return t;
}
unsigned long long& launch_counter() {
    static thread_local unsigned long long n = 0;
    return n;
}
// for the handle-less entry points defined outside this file (frame_pack.hip): what soccdpt_last_error(NULL) returns
void set_last_error(const std::string& msg) { g_create_error = msg; }
}  // namespace soccdpt

static double occ_cells(const soccdpt_config& c) { return (double)c.grid[0] * c.grid[1] * c.grid[2] * c.num_classes; }

static int fail(Handle* h, const std::string& msg) {
    if (h) h->err = msg; else g_create_error = msg;
    return 1;
}

// ---- profiled launches: each profiler family's name and algorithmic HBM bytes exist here once; the stage-level entry points and the
// two whole-forward entry points launch through them ----
static int profiled_project(Handle* h, const float* inv, const float* seg, int B, int in_h, int in_w, float* inv_up, float* seg_up, float* points,
                            uint32_t* occ_bits, int clear_bits, hipStream_t st) {
    const soccdpt_config& c = h->cfg;
    // inputs once + every requested output once
    const double px = (double)c.cam_width * c.cam_height * B;
    const double bytes = (double)B * in_h * in_w * 4.0 * (1 + c.num_classes) + px * 4.0 * ((inv_up ? 1 : 0) + (seg_up ? c.num_classes : 0) + (points ? 3 : 0));
    ProfScope ps(h->prof, "project_voxelise", 0.0, bytes, st);
    return launch_project(c, inv, seg, B, in_h, in_w, inv_up, seg_up, points, occ_bits, clear_bits, st, h->err);
}
static int profiled_occ_expand(Handle* h, const uint32_t* bits, int B, float* occ, hipStream_t st) {
    ProfScope ps(h->prof, "occ_expand", 0.0, occ_cells(h->cfg) * (4.0 * B + 0.125), st);
    return launch_occ_expand(h->cfg, bits, B, occ, st, h->err);
}
static int profiled_voxelise_frames(Handle* h, const float* inv_up, const float* seg, int B, int in_h, int in_w, uint32_t* frame_bits, int clear_bits,
                                    hipStream_t st) {
    const soccdpt_config& c = h->cfg;
    // the inverse depth and the class maps once, the rows' clear
    const double bytes = (double)B * ((double)c.cam_width * c.cam_height * 4.0 + (double)in_h * in_w * 4.0 * c.num_classes + occ_cells(c) * 0.125);
    ProfScope ps(h->prof, "voxelise_frames", 0.0, bytes, st);
    return launch_voxelise_frames(c, inv_up, seg, B, in_h, in_w, frame_bits, clear_bits, st, h->err);
}
static int profiled_occ_expand_frames(Handle* h, const uint32_t* frame_bits, int B, float* occ, hipStream_t st) {
    ProfScope ps(h->prof, "occ_expand_frames", 0.0, occ_cells(h->cfg) * (4.0 + 0.125) * B, st);
    return launch_occ_expand_frames(h->cfg, frame_bits, B, occ, st, h->err);
}

// Head of soccdpt_forward / soccdpt_forward_frames (`who`): the network outputs live at the head of the workspace -- model_network carves its scratch
// behind the same head, so the halo images sit at the same place for every entry point -- and the network runs into them.
static int network_at_head(Handle* h, const char* who, const float* dev_x, int B, void* dev_workspace, size_t workspace_bytes, hipStream_t st, float** inv,
                           float** seg) {
    const int S = h->img;
    *inv = static_cast<float*>(dev_workspace);
    *seg = *inv + (size_t)B * S * S;
    const size_t head = (size_t)B * S * S * (1 + h->cfg.num_classes) * sizeof(float);
    if (workspace_bytes < head) return fail(h, std::string(who) + ": workspace too small");
    return model_network(*h, dev_x, B, *inv, *seg, dev_workspace, workspace_bytes, st, h->err);
}

// soccdpt_prepare found that the precision map in force does not describe the bound weights (or does again): put the map that does in place --
// the shipped one, or x3 operands for every group -- void both caches, whose layout follows the formats, and prepare again.
static int remap_and_prepare(Handle* h, bool shipped_map, void* dev_prepared, size_t prepared_bytes, hipStream_t st) {
    if (shipped_map) model_prec_default(*h);
    else for (const auto& g : model_prec_groups(*h)) h->prec_map[g] = 3;
    h->ws_key = Handle::WsKey();
    model_drop_graph(*h);
    return model_prepare(*h, dev_prepared, prepared_bytes, st, h->err) ? 1 : 0;
}

// The backward passes of the training step (`who`) run with the amp / drop-path modes their forward latched: a setter called between forward
// and backward takes effect at the next forward.
template <class Run>
static int train_backward_as_forward_ran(Handle* h, const char* who, int B, void* dev_workspace, Run&& run) {
    if (h->train_key.ws != dev_workspace || h->train_key.B != B || !dev_workspace)
        return fail(h, std::string(who) + ": no soccdpt_train_forward ran on this workspace with this batch size");
    const int amp_now = h->train_amp;
    const float dp_now = h->train_drop_path;
    h->train_amp = h->train_key.amp; h->train_drop_path = h->train_key.drop_path;
    const int rc = run();
    h->train_amp = amp_now; h->train_drop_path = dp_now;
    return rc;
}

extern "C" {

int soccdpt_abi_version(void) { return SOCCDPT_ABI_VERSION; }
size_t soccdpt_sizeof(int which) {
    switch (which) {
        case 0: return sizeof(soccdpt_config);
        case 1: return sizeof(soccdpt_igemm_args);
        case 2: return sizeof(soccdpt_kernel_stat);
        case 3: return sizeof(soccdpt_calib_report);
        case 4: return sizeof(soccdpt_calib_options);
        case 5: return sizeof(soccdpt_train_layer_bwd_args);
        case 6: return sizeof(soccdpt_train_aux_args);
        case 7: return sizeof(soccdpt_fwd_aux_args);
        default: return 0;
    }
}

int soccdpt_prec_map_set(void* handle, const char* group, int fmt) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h || !group) return -1;
    if (h->cfg.precision != SOCCDPT_PREC_MIXED) { fail(h, "soccdpt_prec_map_set: the handle was not created with SOCCDPT_PREC_MIXED"); return -1; }
    if (fmt != SOCCDPT_PREC_F16 && fmt != SOCCDPT_PREC_F16X3 && fmt != SOCCDPT_PREC_F16X2W) { fail(h, "soccdpt_prec_map_set: fmt must be SOCCDPT_PREC_F16, SOCCDPT_PREC_F16X2W or SOCCDPT_PREC_F16X3"); return -1; }
    const int n = model_prec_set(*h, group, fmt == SOCCDPT_PREC_F16X3 ? 3 : (fmt == SOCCDPT_PREC_F16X2W ? 4 : 1), h->err);
    if (n < 0) return n;
    // formats decide where the zero borders of the 3x3 inputs lie and which weight copies exist: both caches are void
    h->ws_key = Handle::WsKey();
    h->is_prepared = false;
    h->prec_source = 2;   // edited by the caller
    model_drop_graph(*h);
    return n;
}
int soccdpt_prec_map_get(void* handle, char* buf, int buf_bytes) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return -1;
    std::string out;
    for (const auto& g : model_prec_groups(*h)) {
        auto it = h->prec_map.find(g);
        const int f = h->cfg.precision == SOCCDPT_PREC_MIXED ? (it == h->prec_map.end() ? SOCCDPT_PREC_F16 : it->second == 3 ? SOCCDPT_PREC_F16X3 : it->second == 4 ? SOCCDPT_PREC_F16X2W : SOCCDPT_PREC_F16)
                                                             : h->cfg.precision;
        if (!out.empty()) out += ' ';
        out += g + "=" + std::to_string(f);
    }
    if (buf && buf_bytes > 0) {
        const size_t n = out.size() < (size_t)buf_bytes - 1 ? out.size() : (size_t)buf_bytes - 1;
        memcpy(buf, out.data(), n);
        buf[n] = 0;
    }
    return (int)out.size();
}

int soccdpt_create(const soccdpt_config* cfg, void** handle) {
    if (!cfg || !handle) return fail(nullptr, "soccdpt_create: null argument");
    if (cfg->abi_version != SOCCDPT_ABI_VERSION) return fail(nullptr, "soccdpt_create: abi_version mismatch");
    if (cfg->num_classes != 3) return fail(nullptr, "soccdpt_create: num_classes must be 3 (model/SOccDPT.py:347-349)");
    if (cfg->features != 256) return fail(nullptr, "soccdpt_create: features must be 256");
    if (cfg->cam_width <= 0 || cfg->cam_height <= 0) return fail(nullptr, "soccdpt_create: bad camera size");
    if (cfg->precision != SOCCDPT_PREC_BF16 && cfg->precision != SOCCDPT_PREC_F32 && cfg->precision != SOCCDPT_PREC_F16 && cfg->precision != SOCCDPT_PREC_F16X3 &&
        cfg->precision != SOCCDPT_PREC_MIXED)
        return fail(nullptr, "soccdpt_create: unknown precision");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, "soccdpt_create: no HIP device visible (the MI355X path has no CPU fallback)");
    Handle* h = new Handle();
    if (const char* e = getenv("SOCCDPT_MLP_FUSE_MAX")) h->mlp_fuse_max = atoi(e);   // measurement switch (0 = unfused everywhere)
    if (const char* e = getenv("SOCCDPT_FUSE_QKV")) h->fuse_qkv = atoi(e) != 0;         // measurement switch: 0 = qkv igemm + window_attention as in rounds 1-5
    if (const char* e = getenv("SOCCDPT_FUSE_QKV_STAGES")) h->fuse_qkv_mask = atoi(e);
    h->cfg = *cfg;
    (void)hipGetDevice(&h->device);
    std::string err;
    if (model_init(*h, err)) {
        delete h;
        return fail(nullptr, err);
    }
    *handle = h;
    return 0;
}

void soccdpt_destroy(void* handle) { delete static_cast<Handle*>(handle); }

const char* soccdpt_last_error(void* handle) {
    return handle ? static_cast<Handle*>(handle)->err.c_str() : g_create_error.c_str();
}

int soccdpt_bind_weight(void* handle, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h || !key || !dev_ptr) return fail(h, "soccdpt_bind_weight: null argument");
    if (dtype != SOCCDPT_DTYPE_F32) return fail(h, std::string("soccdpt_bind_weight: only f32 tensors are accepted: ") + key);
    return model_bind(*h, key, dev_ptr, shape, ndim, h->err);
}

int soccdpt_num_weights(void* handle) { return (int)static_cast<Handle*>(handle)->weights.size(); }
const char* soccdpt_weight_key(void* handle, int index) {
    Handle* h = static_cast<Handle*>(handle);
    if (index < 0 || index >= (int)h->weights.size()) return nullptr;
    return h->weights[index].key.c_str();
}

size_t soccdpt_prepared_bytes(void* handle) { return static_cast<Handle*>(handle)->prepared_bytes; }
size_t soccdpt_workspace_bytes(void* handle, int B) { return model_workspace_bytes(*static_cast<Handle*>(handle), B); }
int soccdpt_workspace_invalidate(void* handle) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    h->ws_key = Handle::WsKey();
    model_drop_graph(*h);
    return 0;
}
int soccdpt_workspace_zero_fills(void* handle) { return handle ? static_cast<Handle*>(handle)->ws_zero_fills : -1; }

int soccdpt_prepare(void* handle, void* dev_prepared, size_t prepared_bytes, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    if (model_prepare(*h, dev_prepared, prepared_bytes, (hipStream_t)stream, h->err)) return 1;
    // the fingerprint kernels' 8 bytes of output: the arena's 256-byte tail is free
    unsigned long long* tmp = reinterpret_cast<unsigned long long*>((reinterpret_cast<uintptr_t>(dev_prepared) + h->prepared_bytes - 8) & ~uintptr_t(7));
    if (h->cfg.precision == SOCCDPT_PREC_MIXED && h->prec_source == 1 && h->calib_fp_valid) {
        // A calibrated map is a statement about the weights it was derived on: other values under the same keys -- a rebind, or a
        // load_state_dict / optimizer step into the same storage -- void it.  Same four-tensor fingerprint as below; on a mismatch every group
        // goes back to x3 operands (source 3) until the caller calibrates again.
        unsigned long long fp = 0;
        const int rc = calib_fingerprint(*h, tmp, (hipStream_t)stream, &fp, h->err);
        if (rc < 0) return 1;
        if (rc > 0 || fp != h->calib_fp) {
            h->prec_source = 3;
            h->calib_fp_valid = false;
            return remap_and_prepare(h, false, dev_prepared, prepared_bytes, (hipStream_t)stream);
        }
        return 0;
    }
    if (h->cfg.precision == SOCCDPT_PREC_MIXED && h->prec_source != 1 && h->prec_source != 2) {
        // Is the shipped map running on the weights it was derived from?  (a fingerprint of four tensors.)
        // On any other weights its within-tolerance claim is unverified -- measured in round 5: a second synthetic draw leaves the class logits at
        // 1.4e-3 under the shipped map -- so until soccdpt_prec_calibrate has run every group takes x3 operands (f32-grade, about 1.7x the step).
        const int same = calib_weights_are_the_shipped_draw(*h, tmp, (hipStream_t)stream, h->err);
        if (same < 0) return 1;
        const int was = h->prec_source;
        h->prec_source = same ? 0 : 3;
        if (h->prec_source != was && (h->prec_source == 3 || was == 3)) return remap_and_prepare(h, same != 0, dev_prepared, prepared_bytes, (hipStream_t)stream);
    }
    return 0;
}

size_t soccdpt_prec_calibrate_scratch_bytes(void* handle, int B) { return handle ? calib_scratch_bytes(*static_cast<Handle*>(handle), B) : 0; }
int soccdpt_prec_calibrate(void* handle, const float* dev_x, int B, float budget, void* dev_prepared, size_t prepared_bytes, void* dev_workspace,
                           size_t workspace_bytes, void* dev_scratch, size_t scratch_bytes, soccdpt_calib_report* report, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    soccdpt_calib_options opt;
    memset(&opt, 0, sizeof(opt));
    opt.struct_bytes = (int32_t)sizeof(opt);
    opt.budget = budget;
    return calib_run(*h, dev_x, B, opt, dev_prepared, prepared_bytes, dev_workspace, workspace_bytes, dev_scratch, scratch_bytes, report, (hipStream_t)stream, h->err);
}
int soccdpt_prec_calibrate_ex(void* handle, const float* dev_x, int B, const soccdpt_calib_options* options, void* dev_prepared, size_t prepared_bytes,
                              void* dev_workspace, size_t workspace_bytes, void* dev_scratch, size_t scratch_bytes, soccdpt_calib_report* report, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    if (!options || options->struct_bytes != (int32_t)sizeof(soccdpt_calib_options)) return fail(h, "soccdpt_prec_calibrate_ex: options missing or compiled against another header (struct_bytes)");
    return calib_run(*h, dev_x, B, *options, dev_prepared, prepared_bytes, dev_workspace, workspace_bytes, dev_scratch, scratch_bytes, report, (hipStream_t)stream, h->err);
}
int soccdpt_prec_map_source(void* handle) {
    Handle* h = static_cast<Handle*>(handle);
    return (h && h->cfg.precision == SOCCDPT_PREC_MIXED) ? h->prec_source : -1;
}

int soccdpt_network(void* handle, const float* dev_x, int B, float* dev_inv256, float* dev_seg256, void* dev_workspace,
                    size_t workspace_bytes, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    return model_network(*h, dev_x, B, dev_inv256, dev_seg256, dev_workspace, workspace_bytes, (hipStream_t)stream, h->err);
}

int soccdpt_bind_grad(void* handle, const char* key, float* dev_grad) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h || !key) return fail(h, "soccdpt_bind_grad: null argument");
    auto it = h->index.find(key);
    if (it == h->index.end()) return fail(h, std::string("soccdpt_bind_grad: unknown key: ") + key);
    h->weights[it->second].grad = dev_grad;
    return 0;
}
int soccdpt_train_set_amp(void* handle, int on) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    if (on < 0 || on > 3) return fail(h, "soccdpt_train_set_amp: mode must be 0 (off), 1 (bf16), 2 (fp16) or 3 (x3 split fp16)");
    h->train_amp = on;
    return 0;
}
int soccdpt_train_set_drop_path(void* handle, float rate) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    if (!(rate >= 0.f && rate < 1.f)) return fail(h, "soccdpt_train_set_drop_path: rate must be in [0, 1)");
    h->train_drop_path = rate;
    return 0;
}

int soccdpt_train_unscale(float* dev_grads, size_t n, float inv_scale, int* dev_found_inf, void* stream) {
    if (!dev_grads || !dev_found_inf) return fail(nullptr, "soccdpt_train_unscale: null argument");
    if (n == 0) return 0;
    std::string err;
    if (tr_unscale_check(dev_grads, n, inv_scale, dev_found_inf, (hipStream_t)stream, err)) return fail(nullptr, err);
    return 0;
}
size_t soccdpt_train_workspace_bytes(void* handle, int B) { return handle && B > 0 ? train_workspace_bytes(*static_cast<Handle*>(handle), B) : 0; }
int soccdpt_train_backward_encoder(void* handle, int B, const float* const* dev_d_feat, void* dev_workspace, size_t workspace_bytes, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    return train_backward_as_forward_ran(h, "soccdpt_train_backward_encoder", B, dev_workspace, [&] {
        return train_backward_encoder(*h, B, dev_d_feat, dev_workspace, workspace_bytes, (hipStream_t)stream, h->err);
    });
}
int soccdpt_train_workspace_tensor(void* handle, int B, const char* name, size_t* byte_offset, size_t* elems) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h || !byte_offset || !elems) return 1;
    return train_workspace_tensor(*h, B, name, byte_offset, elems);
}
int soccdpt_train_forward(void* handle, const float* dev_x, int B, float* dev_inv, float* dev_seg, void* dev_workspace, size_t workspace_bytes,
                          float dropout_p, uint32_t seed, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    if (!dev_x || !dev_inv || !dev_seg) return fail(h, "soccdpt_train_forward: null argument");
    if (!(dropout_p >= 0.f && dropout_p < 1.f)) return fail(h, "soccdpt_train_forward: dropout_p must be in [0, 1)");
    h->train_key = Handle::TrainKey();
    if (train_forward(*h, dev_x, B, dev_inv, dev_seg, dev_workspace, workspace_bytes, dropout_p, seed, (hipStream_t)stream, h->err)) return 1;
    h->train_key.ws = dev_workspace; h->train_key.B = B; h->train_key.dropout_p = dropout_p;
    h->train_key.amp = h->train_amp; h->train_key.drop_path = h->train_drop_path;
    return 0;
}
int soccdpt_train_backward(void* handle, const float* dev_x, int B, const float* dev_d_inv, const float* dev_d_seg, void* dev_workspace,
                           size_t workspace_bytes, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    if (!dev_d_inv || !dev_d_seg) return fail(h, "soccdpt_train_backward: null argument");
    return train_backward_as_forward_ran(h, "soccdpt_train_backward", B, dev_workspace, [&] {
        return train_backward(*h, dev_x, B, dev_d_inv, dev_d_seg, dev_workspace, workspace_bytes, (hipStream_t)stream, h->err);
    });
}

int soccdpt_project(void* handle, const float* dev_inv, const float* dev_seg, int B, int in_h, int in_w, float* dev_inv_up,
                    float* dev_seg_up, float* dev_points, uint32_t* dev_occ_bits, int clear_bits, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    if (!dev_inv || !dev_seg) return fail(h, "soccdpt_project: null input");
    return profiled_project(h, dev_inv, dev_seg, B, in_h, in_w, dev_inv_up, dev_seg_up, dev_points, dev_occ_bits, clear_bits, (hipStream_t)stream);
}

size_t soccdpt_occ_words(void* handle) {
    Handle* h = static_cast<Handle*>(handle);
    const size_t ncell = (size_t)h->cfg.grid[0] * h->cfg.grid[1] * h->cfg.grid[2] * h->cfg.num_classes;
    return (ncell + 31) / 32;
}

size_t soccdpt_project_backward_scratch_bytes(void* handle, int B, int in_h) {
    Handle* h = static_cast<Handle*>(handle);
    return (h && B > 0 && in_h > 0) ? upsample_bwd_scratch_bytes(h->cfg, B, in_h) : 0;
}

int soccdpt_project_backward(void* handle, const float* dev_inv_up, const float* dev_d_inv_up, const float* dev_d_seg_up, const float* dev_d_points,
                             int B, int in_h, int in_w, float* dev_d_inv, float* dev_d_seg, void* dev_scratch, size_t scratch_bytes, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    if (B <= 0 || in_h <= 0 || scratch_bytes < upsample_bwd_scratch_bytes(h->cfg, B, in_h)) return fail(h, "soccdpt_project_backward: scratch too small");
    if (launch_upsample_bwd(h->cfg, dev_inv_up, dev_d_inv_up, dev_d_seg_up, dev_d_points, B, in_h, in_w, dev_d_inv, dev_d_seg, dev_scratch,
                            (hipStream_t)stream, h->err))
        return 1;
    return 0;
}

int soccdpt_occ_or(void* handle, uint32_t* dev_dst_bits, const uint32_t* dev_src_bits, int n_sets, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    if (n_sets <= 0) return 0;
    return launch_occ_or(h->cfg, dev_dst_bits, dev_src_bits, n_sets, (hipStream_t)stream, h->err);
}

int soccdpt_occ_expand(void* handle, const uint32_t* dev_bits, int B, float* dev_occ, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    if (B <= 0) return fail(h, "soccdpt_occ_expand: empty batch");
    return profiled_occ_expand(h, dev_bits, B, dev_occ, (hipStream_t)stream);
}

int soccdpt_occ_zero(void* handle, int B, float* dev_occ, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    if (B <= 0 || !dev_occ) return fail(h, "soccdpt_occ_zero: bad argument");
    ProfScope ps(h->prof, "occ_zero", 0.0, occ_cells(h->cfg) * 4.0 * B, (hipStream_t)stream);
    return launch_occ_zero(h->cfg, B, dev_occ, (hipStream_t)stream, h->err);
}

int soccdpt_occ_set(void* handle, const uint32_t* dev_bits, int B, float* dev_occ, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    if (B <= 0 || !dev_occ || !dev_bits) return fail(h, "soccdpt_occ_set: bad argument");
    ProfScope ps(h->prof, "occ_set", 0.0, occ_cells(h->cfg) * 0.125, (hipStream_t)stream);
    return launch_occ_set(h->cfg, dev_bits, B, dev_occ, (hipStream_t)stream, h->err);
}

int soccdpt_forward(void* handle, const float* dev_x, int B, float* dev_inv_up, float* dev_seg_up, float* dev_points,
                    float* dev_occ, uint32_t* dev_occ_bits, void* dev_workspace, size_t workspace_bytes, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    if (B <= 0) return fail(h, "soccdpt_forward: empty batch");
    const int S = h->img;
    hipStream_t st = (hipStream_t)stream;
    float *inv, *seg;
    int rc = network_at_head(h, "soccdpt_forward", dev_x, B, dev_workspace, workspace_bytes, st, &inv, &seg);
    if (rc) return rc;
    const bool occ_on = h->cfg.compute_occ != 0;
    if (occ_on && !dev_occ_bits) return fail(h, "soccdpt_forward: compute_occ needs dev_occ_bits");
    rc = profiled_project(h, inv, seg, B, S, S, dev_inv_up, dev_seg_up, dev_points, occ_on ? dev_occ_bits : nullptr, 1, st);
    if (rc) return rc;
    if (occ_on && dev_occ) rc = profiled_occ_expand(h, dev_occ_bits, B, dev_occ, st);
    return rc;
}

int soccdpt_voxelise_frames(void* handle, const float* dev_inv_up, const float* dev_seg, int B, int in_h, int in_w, uint32_t* dev_frame_bits,
                            int clear_bits, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    if (!dev_inv_up || !dev_seg || !dev_frame_bits) return fail(h, "soccdpt_voxelise_frames: null argument");
    if (B <= 0 || in_h <= 0 || in_w <= 0) return fail(h, "soccdpt_voxelise_frames: empty input");
    return profiled_voxelise_frames(h, dev_inv_up, dev_seg, B, in_h, in_w, dev_frame_bits, clear_bits, (hipStream_t)stream);
}

int soccdpt_occ_expand_frames(void* handle, const uint32_t* dev_frame_bits, int B, float* dev_occ, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    if (!dev_frame_bits || !dev_occ) return fail(h, "soccdpt_occ_expand_frames: null argument");
    if (B <= 0) return fail(h, "soccdpt_occ_expand_frames: empty batch");
    return profiled_occ_expand_frames(h, dev_frame_bits, B, dev_occ, (hipStream_t)stream);
}

int soccdpt_forward_frames(void* handle, const float* dev_x, int B, float* dev_inv_up, float* dev_seg_up, float* dev_points, float* dev_occ,
                           uint32_t* dev_occ_bits, uint32_t* dev_frame_bits, void* dev_workspace, size_t workspace_bytes, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    if (B <= 0) return fail(h, "soccdpt_forward_frames: empty batch");
    if (!dev_x || !dev_workspace) return fail(h, "soccdpt_forward_frames: null argument");
    if (!h->cfg.compute_occ) return fail(h, "soccdpt_forward_frames: the handle was created without compute_occ");
    if (!dev_inv_up) return fail(h, "soccdpt_forward_frames: dev_inv_up is required (the per-frame voxelisation reads the inverse depth back)");
    if (!dev_frame_bits) return fail(h, "soccdpt_forward_frames: dev_frame_bits is required");
    const int S = h->img;
    hipStream_t st = (hipStream_t)stream;
    // always eager: the per-frame passes read this call's outputs, and a captured network graph is keyed on soccdpt_forward's pointers
    const bool graph_was = h->use_graph;
    h->use_graph = false;
    float *inv, *seg;
    int rc = network_at_head(h, "soccdpt_forward_frames", dev_x, B, dev_workspace, workspace_bytes, st, &inv, &seg);
    h->use_graph = graph_was;
    if (rc) return rc;
    // the union comes from the frame rows below, so the fused kernel skips its own marking
    rc = profiled_project(h, inv, seg, B, S, S, dev_inv_up, dev_seg_up, dev_points, nullptr, 0, st);
    if (rc) return rc;
    rc = profiled_voxelise_frames(h, dev_inv_up, seg, B, S, S, dev_frame_bits, 1, st);
    if (rc) return rc;
    if (dev_occ_bits) {
        const size_t wbytes = soccdpt_occ_words(h) * sizeof(uint32_t);
        if (hipMemsetAsync(dev_occ_bits, 0, wbytes, st) != hipSuccess) return fail(h, "soccdpt_forward_frames: clearing dev_occ_bits failed");
        ProfScope ps(h->prof, "occ_or", 0.0, occ_cells(h->cfg) * 0.125 * (B + 2), st);
        rc = launch_occ_or(h->cfg, dev_occ_bits, dev_frame_bits, B, st, h->err);
        if (rc) return rc;
    }
    if (dev_occ) rc = profiled_occ_expand_frames(h, dev_frame_bits, B, dev_occ, st);
    return rc;
}

int soccdpt_last_launch_count(void* handle) { return static_cast<Handle*>(handle)->launches; }
unsigned long long soccdpt_launch_counter(void) { return soccdpt::launch_counter(); }

size_t soccdpt_metrics_scratch_bytes(int B, int C) { return metrics_scratch_bytes(B, C); }

int soccdpt_metrics_depth(const float* dev_pred, const float* dev_gt, const uint8_t* dev_mask, int B, size_t npix, float* dev_out,
                          void* dev_scratch, void* stream) {
    std::string err;
    if (!dev_pred || !dev_gt || !dev_mask || !dev_out || !dev_scratch) return fail(nullptr, "soccdpt_metrics_depth: null argument");
    if (launch_depth_metrics(dev_pred, dev_gt, dev_mask, B, npix, dev_out, dev_scratch, (hipStream_t)stream, err)) return fail(nullptr, err);
    return 0;
}

int soccdpt_metrics_iou(const float* dev_pred, const float* dev_gt, int B, int C, size_t npix, float* dev_out, void* dev_scratch,
                        void* stream) {
    std::string err;
    if (!dev_pred || !dev_gt || !dev_out || !dev_scratch) return fail(nullptr, "soccdpt_metrics_iou: null argument");
    if (launch_iou_metrics(dev_pred, dev_gt, B, C, npix, dev_out, dev_scratch, (hipStream_t)stream, err)) return fail(nullptr, err);
    return 0;
}

int soccdpt_occ_pack(const void* dev_dense, int dtype, int rows, size_t ncell, float threshold, int strict, uint32_t* dev_bits, void* stream) {
    std::string err;
    if (launch_occ_pack(dev_dense, dtype, rows, ncell, threshold, strict, dev_bits, (hipStream_t)stream, err)) return fail(nullptr, "soccdpt_" + err);
    return 0;
}

size_t soccdpt_occ_points_scratch_bytes(int rows, size_t ncell, int C) { return occ_points_scratch_bytes(rows, ncell, C); }

int soccdpt_occ_points_count(const uint32_t* dev_bits, int rows, size_t ncell, int C, void* dev_scratch, size_t scratch_bytes, int64_t* dev_counts,
                             int64_t* dev_total, void* stream) {
    std::string err;
    if (launch_occ_points_count(dev_bits, rows, ncell, C, dev_scratch, scratch_bytes, dev_counts, dev_total, (hipStream_t)stream, err))
        return fail(nullptr, "soccdpt_" + err);
    return 0;
}

int soccdpt_occ_points_write(const uint32_t* dev_bits, int rows, const int32_t* grid, int C, const float* occupancy_shape, const void* dev_scratch,
                             size_t scratch_bytes, size_t capacity, double* dev_points, const uint8_t* dev_class_colors, uint8_t* dev_colors,
                             void* stream) {
    std::string err;
    if (launch_occ_points_write(dev_bits, rows, grid, C, occupancy_shape, dev_scratch, scratch_bytes, capacity, dev_points, dev_class_colors, dev_colors,
                                (hipStream_t)stream, err))
        return fail(nullptr, "soccdpt_" + err);
    return 0;
}

int soccdpt_occ_iou_counts(const uint32_t* dev_pred_bits, int pred_rows, const uint32_t* dev_gt_bits, int rows, size_t ncell, int C,
                           uint64_t* dev_counts, void* stream) {
    std::string err;
    if (launch_occ_iou_counts(dev_pred_bits, pred_rows, dev_gt_bits, rows, ncell, C, dev_counts, (hipStream_t)stream, err))
        return fail(nullptr, "soccdpt_" + err);
    return 0;
}

int soccdpt_set_streams(void* handle, int n) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    if (n > 1) {   // experimental: see the header
        const char* e = getenv("SOCCDPT_ALLOW_MULTISTREAM");
        if (!e || atoi(e) != 1) return fail(h, "soccdpt_set_streams: n > 1 is experimental (DESIGN.md section 4); set SOCCDPT_ALLOW_MULTISTREAM=1 to opt in");
    }
    h->ws_key = Handle::WsKey();
    return model_set_streams(*h, n, h->err);
}

int soccdpt_set_graph(void* handle, int on) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    if (on && !h->graph_stream) {
        if (hipStreamCreateWithFlags(&h->graph_stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&h->graph_in, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&h->graph_out, hipEventDisableTiming) != hipSuccess)
            return fail(h, "soccdpt_set_graph: stream/event creation failed");
    }
    h->use_graph = on != 0;
    if (!h->use_graph) model_drop_graph(*h);
    return 0;
}

int soccdpt_profile_enable(void* handle, int on) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    h->prof.on = on != 0;
    h->prof.recs.clear();
    h->prof.used = 0;
    return 0;
}

int soccdpt_profile_collect(void* handle, soccdpt_kernel_stat* out, int max_entries, int* n_entries) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h || !out || !n_entries) return 1;
    int n = 0;
    for (const ProfRec& r : h->prof.recs) {
        float ms = 0.f;
        for (size_t i = r.first_pair; i < r.first_pair + r.n_pairs; ++i) {   // each pair is bound to one dispatch: stop - start = the kernel's own duration
            hipEvent_t e0 = h->prof.pool[2 * i], e1 = h->prof.pool[2 * i + 1];
            if (hipEventSynchronize(e1) != hipSuccess) return fail(h, "soccdpt_profile_collect: event sync failed");
            float t = 0.f;
            if (hipEventElapsedTime(&t, e0, e1) != hipSuccess) return fail(h, "soccdpt_profile_collect: elapsed failed");
            ms += t;
        }
        int k = 0;
        for (; k < n; ++k)
            if (!std::strcmp(out[k].name, r.name)) break;
        if (k == n) {
            if (n == max_entries) continue;
            std::memset(&out[n], 0, sizeof(out[n]));
            std::strncpy(out[n].name, r.name, sizeof(out[n].name) - 1);
            ++n;
        }
        out[k].launches += (int)r.n_pairs;
        out[k].ms += ms;
        out[k].flops += r.flops;
        out[k].bytes += r.bytes;
    }
    *n_entries = n;
    h->prof.recs.clear();
    h->prof.used = 0;
    return 0;
}

int soccdpt_profile_sites(void* handle, int on) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    h->prof_sites = on != 0;
    h->sites.clear();
    h->sites.reserve(1024);   // the profiler records keep pointers to SiteRec::name: no reallocation while profiling
    return 0;
}
int soccdpt_site_count(void* handle) {
    Handle* h = static_cast<Handle*>(handle);
    return h ? (int)h->sites.size() : 0;
}
int soccdpt_site_get(void* handle, int i, int* M, int* N, int* K, int* taps, int* cfg, int* launches) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h || i < 0 || i >= (int)h->sites.size()) return 1;
    const SiteRec& r = h->sites[i];
    *M = r.M; *N = r.N; *K = r.K; *taps = r.taps; *cfg = r.cfg; *launches = r.count;
    return 0;
}
int soccdpt_tune_set(void* handle, int M, int N, int K, int taps, int cfg) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    const long long key = (((long long)M * 8192 + N) * 65536 + K) * 16 + taps;
    if (cfg < 0) h->tune_by_shape.erase(key);
    else h->tune_by_shape[key] = cfg;
    model_drop_graph(*h);
    return 0;
}
int soccdpt_tune_clear(void* handle) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return 1;
    h->tune_by_shape.clear();
    model_drop_graph(*h);
    return 0;
}

int soccdpt_gt_occupancy(int B, int H, int W, int C, const double* intr, const double* pc_scale, const double* pc_shift,
                         const double* rot27, const float* occ_shape, const int* grid, float threshold, const float* disparity,
                         const int32_t* seg_class, float* depth, double* points, uint32_t* counts, uint8_t* occ, void* stream) {
    std::string err;
    if (launch_gt_occupancy(B, H, W, C, intr, pc_scale, pc_shift, rot27, occ_shape, grid, threshold, disparity, seg_class, depth, points, counts, occ,
                            (hipStream_t)stream, err))
        return fail(nullptr, err);
    return 0;
}

int soccdpt_input_transform_u8(const uint8_t* img, int B, int Hs, int Ws, int Hd, int Wd, const double* mean, const double* stdv, float* out,
                               void* stream) {
    std::string err;
    if (launch_input_transform_u8(img, B, Hs, Ws, Hd, Wd, mean, stdv, out, (hipStream_t)stream, err)) return fail(nullptr, err);
    return 0;
}

int soccdpt_op_mlp_ln(const void* x_op, float* x_f32, const void* w1, const float* b1, const void* w2, const float* b2, const float* ln_g,
                      const float* ln_b, void* x_op_out, void* halo, int precision, int M, int C, int H, int W, int merge, void* stream) {
    std::string err;
    if (precision != SOCCDPT_PREC_BF16 && precision != SOCCDPT_PREC_F16) return fail(nullptr, "soccdpt_op_mlp_ln: 16-bit operand modes only");
    if (launch_mlp_ln(static_cast<const bf16_t*>(x_op), x_f32, static_cast<const bf16_t*>(w1), b1, static_cast<const bf16_t*>(w2), b2, ln_g, ln_b,
                      static_cast<bf16_t*>(x_op_out), static_cast<bf16_t*>(halo), precision == SOCCDPT_PREC_F16, M, C, H, W, merge ? 1 : 0, (hipStream_t)stream, err))
        return fail(nullptr, err);
    return 0;
}

int soccdpt_adam_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                      float* const* exp_avg_sq, const size_t* sizes, double lr, double beta1, double beta2, double eps,
                      double weight_decay, int step, void* stream) {
    std::string err;
    if (launch_adam(n_tensors, params, grads, exp_avg, exp_avg_sq, sizes, lr, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream, err))
        return fail(nullptr, err);
    return 0;
}

size_t soccdpt_loss_scratch_bytes(int B, int H, int W, int h, int w) { return loss_scratch_bytes(B, H, W, h, w); }

int soccdpt_training_loss(int B, int H, int W, int h, int w, int C, int compute_scale_and_shift, float alpha, float loss_depth_w,
                          float loss_seg_w, const float* inv, const float* seg, const float* y_disp, const uint8_t* mask_disp,
                          const float* y_seg, const uint8_t* mask_seg, float* out, float* d_inv, float* d_seg, void* scratch,
                          void* stream) {
    std::string err;
    if (launch_training_loss(B, H, W, h, w, C, compute_scale_and_shift, alpha, loss_depth_w, loss_seg_w, inv, seg, y_disp, mask_disp, y_seg,
                             mask_seg, out, d_inv, d_seg, scratch, (hipStream_t)stream, err))
        return fail(nullptr, err);
    return 0;
}

int soccdpt_op_igemm(const soccdpt_igemm_args* a, void* stream) {
    if (!a) return fail(nullptr, "soccdpt_op_igemm: null args");
    IgemmDesc d;
    d.X = a->x; d.Wt = a->wt;
    d.M = a->M; d.N = a->N; d.Cin = a->Cin; d.taps = a->taps; d.ldx = a->ldx; d.H = a->H; d.W = a->W;
    d.bias = a->bias; d.res1 = a->res1; d.res2 = a->res2; d.act = a->act; d.out_f32 = a->out_f32; d.act_on_f32 = a->act_on_f32;
    d.out_op = a->out_bf16; d.f32 = a->precision == SOCCDPT_PREC_F32; d.f16 = a->precision == SOCCDPT_PREC_F16; d.x3 = a->precision == SOCCDPT_PREC_F16X3; d.x2w = a->precision == SOCCDPT_PREC_F16X2W; if (d.x2w) d.f16 = 1; d.out_halo = a->out_halo; d.dot_w = a->dot_w; d.dot_b = a->dot_b; d.out_dot = a->out_dot; d.tune = a->tune;
    d.splitk = a->splitk > 1 ? a->splitk : 1; d.sk_part = a->sk_part; d.sk_count = a->sk_count;
    d.sk_part_floats = a->sk_part_floats; d.sk_count_words = a->sk_count_words; d.sk_defer = a->sk_defer;
    if (a->conv_general) { d.stride = a->stride; d.pad = a->pad; d.in_halo = a->in_halo; d.Hi = a->Hi; d.Wi = a->Wi; d.gather1 = a->gather1; }
    d.grp_rows = a->grp_rows; d.grp_off = a->grp_off; d.grp_stride = a->grp_stride; d.seg2_k = a->seg2_k; d.seg2_off = a->seg2_off;
    int gn_bm = 0;
    d.gn_stats = a->gn_stats; d.gn_part = a->gn_part; d.gn_bm_out = &gn_bm; d.gn_cpg = a->gn_cpg; d.gn_hw = a->gn_hw;
    d.gn_part_floats = a->gn_part_floats;
    d.stamps = reinterpret_cast<unsigned long long*>(a->stamps);
    // ABI 6: the fused epilogues (zeros / NULLs: the generic epilogue, operand copies in the launch's own format)
    d.res2_h = a->res2_h; d.res2_w = a->res2_w;
    d.ln_g = a->ln_g; d.ln_b = a->ln_b; d.ln_xf = a->ln_xf; d.ln_halo = a->ln_halo; d.ln_residual = a->ln_residual;
    d.dot3 = a->dot3;
    d.out_fmt = a->out_fmt == 0 ? -1 : a->out_fmt; d.halo_fmt = a->halo_fmt == 0 ? -1 : a->halo_fmt;
    if ((a->res2_h != 0 || a->res2_w != 0) && (a->res2_h <= 0 || a->res2_w <= 0 || !a->res2))
        return fail(nullptr, "soccdpt_op_igemm: a sampled residual needs res2 and its source size (res2_h, res2_w > 0)");
    if (a->res2_h && (a->ln_g || a->dot3)) return fail(nullptr, "soccdpt_op_igemm: the sampled residual belongs to the generic epilogue");
    if (a->ln_g && (a->res1 || a->res2 || a->act || a->out_f32 || a->out_halo || a->dot3 || a->out_dot))
        return fail(nullptr, "soccdpt_op_igemm: the LayerNorm epilogue writes ln_xf / out_bf16 / ln_halo only (no res1, res2, act, out_f32, out_halo or dot)");
    if (a->ln_halo && !a->ln_g) return fail(nullptr, "soccdpt_op_igemm: ln_halo needs the LayerNorm epilogue (ln_g)");
    if (a->ln_g && a->taps != 1) return fail(nullptr, "soccdpt_op_igemm: the LayerNorm epilogue is a plain-GEMM (taps == 1) feature");
    if (a->ln_residual != 0 && a->ln_residual != 1) return fail(nullptr, "soccdpt_op_igemm: ln_residual is 0 or 1");
    if (a->dot3 && (a->taps != 9 || a->Cin % 64 || a->N % 128 || !a->dot_w || !a->out_dot))
        return fail(nullptr, "soccdpt_op_igemm: dot3 needs taps == 9, Cin % 64 == 0, N % 128 == 0, dot_w and out_dot");
    if (a->dot3 && a->precision != SOCCDPT_PREC_BF16 && a->precision != SOCCDPT_PREC_F16)
        return fail(nullptr, "soccdpt_op_igemm: dot3 needs SOCCDPT_PREC_BF16 or _F16 operands");
    if (a->dot3 && a->tune != -1 && a->tune != 21 && a->tune != 47) return fail(nullptr, "soccdpt_op_igemm: dot3 takes tune -1, 21 (128-wide) or 47 (256-wide)");
    for (int f : {a->out_fmt, a->halo_fmt}) {
        const bool same = f == 0 || f == -1;
        const bool to_f16 = f == 1 && a->precision == SOCCDPT_PREC_F16X3;
        const bool to_x3 = f == 3 && (a->precision == SOCCDPT_PREC_F16 || a->precision == SOCCDPT_PREC_F16X2W);
        if (!same && !to_f16 && !to_x3)
            return fail(nullptr, "soccdpt_op_igemm: out_fmt / halo_fmt is -1 or 0 (the launch's format), 1 (fp16 from an x3 launch) or 3 (x3 from an fp16 launch)");
    }
    if (a->halo_fmt > 0 && !a->ln_halo) return fail(nullptr, "soccdpt_op_igemm: halo_fmt without ln_halo");
    std::string err;
    if (a->gn_stats && a->gn_count && (a->gn_hw <= 0 || a->gn_cpg <= 0 || a->M % a->gn_hw || a->N % a->gn_cpg))
        return fail(nullptr, "soccdpt_op_igemm: GroupNorm statistics requested with gn_hw / gn_cpg that do not divide M / N");
    // x3 tile 12 has no generalised-addressing instantiation, and for such a descriptor the tile rule (igemm.hip: pick_cfg_f32) passes tune 12 over and runs
    // tile 4 or 1: at this entry a tune names the tile under test, so the launch is refused
    if (d.x3 && d.tune == 12 && d.splitk <= 1 && !d.ln_g &&
        (d.stride != 1 || d.pad != 1 || d.in_halo != 1 || d.Hi || d.Wi || d.gather1 || d.grp_rows || d.seg2_k || d.stamps))
        return fail(nullptr, "soccdpt_op_igemm: x3 configuration 12 has no generalised addressing");
    if (launch_igemm(d, (hipStream_t)stream, err)) return fail(nullptr, err);
    if (a->gn_stats && a->gn_count && (gn_bm <= 0 || a->gn_hw % gn_bm))
        return fail(nullptr, "soccdpt_op_igemm: statistics requested but the chosen tile has no statistics epilogue (tune forces a tile without one)");
    // gn_count != NULL: the caller wants {mean, rstd} in gn_stats (the form of rounds 2-4, where the convolution's last workgroup finished them; the words of
    // gn_count are no longer touched): a finish launch behind the convolution.  gn_count == NULL: partials only, as the forward launches it.
    if (a->gn_stats && a->gn_count && launch_gn_finish(a->gn_part, a->gn_stats, a->M / a->gn_hw, a->gn_hw / gn_bm, a->N / a->gn_cpg, a->gn_hw, a->gn_cpg, 1e-5f, (hipStream_t)stream, err))
        return fail(nullptr, err);
    return 0;
}

int soccdpt_op_depth_tail(const void* dev_d1, const void* dev_wt, const float* dev_bias, const float* dev_w4, float b4, float* dev_out, int precision,
                          int B, int h, int w, void* stream) {
    std::string err;
    if (!dev_d1 || !dev_wt || !dev_bias || !dev_w4 || !dev_out) return fail(nullptr, "soccdpt_op_depth_tail: null argument");
    if (precision != SOCCDPT_PREC_BF16 && precision != SOCCDPT_PREC_F16) return fail(nullptr, "soccdpt_op_depth_tail: precision is SOCCDPT_PREC_BF16 or _F16");
    if (B <= 0 || h <= 0 || w <= 0) return fail(nullptr, "soccdpt_op_depth_tail: B, h, w must be positive");
    if ((2 * h) % 8 || (2 * w) % 16) return fail(nullptr, "soccdpt_op_depth_tail: the output (2h x 2w) must be a multiple of 8 x 16");
    if (launch_depth_tail(static_cast<const bf16_t*>(dev_d1), static_cast<const bf16_t*>(dev_wt), dev_bias, dev_w4, b4, dev_out, precision == SOCCDPT_PREC_F16 ? 1 : 0,
                          B, h, w, (hipStream_t)stream, err))
        return fail(nullptr, err);
    return 0;
}

int soccdpt_op_seg_tail(const float* dev_part, int nplanes, const float* dev_bias, float* dev_tmp, float* dev_out, int B, int h, int w, int sigmoid,
                        void* stream) {
    std::string err;
    if (!dev_part || !dev_bias || !dev_tmp || !dev_out) return fail(nullptr, "soccdpt_op_seg_tail: null argument");
    if (nplanes < 1 || B <= 0 || h <= 0 || w <= 0) return fail(nullptr, "soccdpt_op_seg_tail: nplanes, B, h and w must be positive");
    if (launch_seg_tail_parts(dev_part, nplanes, dev_bias, dev_tmp, dev_out, B, h, w, sigmoid ? 1 : 0, (hipStream_t)stream, err)) return fail(nullptr, err);
    return 0;
}

int soccdpt_op_wgrad_tn(const void* dev_a, long lda, const void* dev_b, long ldb, size_t K, int Nout, int C, int taps, int rp, int precision, float* dev_scratch,
                        size_t scratch_floats, float* dev_out, void* stream) {
    std::string err;
    if (!dev_a || !dev_b || !dev_scratch || !dev_out) return fail(nullptr, "soccdpt_op_wgrad_tn: null argument");
    if (precision != SOCCDPT_PREC_BF16 && precision != SOCCDPT_PREC_F16 && precision != SOCCDPT_PREC_F16X3) return fail(nullptr, "soccdpt_op_wgrad_tn: bf16, fp16 or f16x3 operands");
    const OpFmt fmt = precision == SOCCDPT_PREC_F16X3 ? OpFmt::X3 : (precision == SOCCDPT_PREC_F16 ? OpFmt::F16 : OpFmt::BF16);
    if (tr_wgrad_tn(dev_a, lda, dev_b, ldb, K, Nout, C, taps, rp, fmt, dev_scratch, scratch_floats, dev_out,
                    (hipStream_t)stream, err))
        return fail(nullptr, err);
    return 0;
}

size_t soccdpt_op_train_layer_bwd_scratch_bytes(const soccdpt_train_layer_bwd_args* args) {
    std::string err;
    const size_t n = args ? train_layer_bwd_scratch_bytes(*args, err) : 0;
    if (!n) fail(nullptr, args ? err : "soccdpt_op_train_layer_bwd_scratch_bytes: null args");
    return n;
}
int soccdpt_op_train_layer_bwd(void* handle, const soccdpt_train_layer_bwd_args* args, void* dev_scratch, size_t scratch_bytes, uint32_t* path_out, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return fail(nullptr, "soccdpt_op_train_layer_bwd: null handle");
    if (!args) return fail(h, "soccdpt_op_train_layer_bwd: null args");
    unsigned path = 0;
    if (train_layer_bwd(*h, *args, dev_scratch, scratch_bytes, &path, (hipStream_t)stream, h->err)) return 1;
    if (path_out) *path_out = path;
    return 0;
}

size_t soccdpt_op_train_aux_scratch_bytes(const soccdpt_train_aux_args* args) {
    std::string err;
    const size_t n = args ? train_aux_scratch_bytes(*args, err) : 0;
    if (!n) fail(nullptr, args ? err : "soccdpt_op_train_aux_scratch_bytes: null args");
    return n;
}
int soccdpt_op_train_aux(const soccdpt_train_aux_args* args, void* dev_scratch, size_t scratch_bytes, void* stream) {
    std::string err;
    if (!args) return fail(nullptr, "soccdpt_op_train_aux: null args");
    if (train_aux(*args, dev_scratch, scratch_bytes, (hipStream_t)stream, err)) return fail(nullptr, err);
    return 0;
}

int soccdpt_op_fwd_aux(const soccdpt_fwd_aux_args* args, uint32_t* path_out, void* stream) {
    std::string err;
    if (!args) return fail(nullptr, "soccdpt_op_fwd_aux: null args");
    unsigned path = 0;
    if (fwd_aux(*args, &path, (hipStream_t)stream, err)) return fail(nullptr, err);
    if (path_out) *path_out = path;
    return 0;
}

// ---- the attention backward of the training step on caller-supplied tensors (tests): no handle, refusals before the first launch ----
static int attn_bwd_fmt(const char* who, int precision, OpFmt* fmt) {
    switch (precision) {
        case SOCCDPT_PREC_F32: *fmt = OpFmt::F32; return 0;
        case SOCCDPT_PREC_BF16: *fmt = OpFmt::BF16; return 0;
        case SOCCDPT_PREC_F16: *fmt = OpFmt::F16; return 0;
        case SOCCDPT_PREC_F16X3: *fmt = OpFmt::X3; return 0;   // the launchers refuse it themselves
        default: return fail(nullptr, std::string(who) + ": unknown precision");
    }
}

int soccdpt_op_attention_bwd_slots(int ws) { return tr_attention_bwd_mfma_slots(ws); }

int soccdpt_op_attention_bwd(const float* dev_qkv, const float* dev_attn_out, const float* dev_dout, const float* dev_cpb_table, const float* dev_scale, float* dev_ds,
                             float* dev_rowstat, float* dev_dscale_part, float* dev_dqkv, int B, int res, int ws, int shift, int heads, int precision, void* stream) {
    std::string err;
    OpFmt fmt;
    if (attn_bwd_fmt("soccdpt_op_attention_bwd", precision, &fmt)) return 1;
    if (tr_attention_bwd_mfma(dev_qkv, dev_attn_out, dev_dout, dev_cpb_table, dev_scale, dev_ds, dev_rowstat, dev_dscale_part, dev_dqkv, B, res, ws, shift, heads,
                              (hipStream_t)stream, err, fmt))
        return fail(nullptr, "soccdpt_op_attention_bwd: " + err);
    return 0;
}

int soccdpt_op_vit_attention_bwd(const float* dev_qkv, const float* dev_attn_out, const float* dev_dout, float* dev_rowstat, float* dev_dqkv, int B, int N, int heads,
                                 int precision, void* stream) {
    std::string err;
    OpFmt fmt;
    if (attn_bwd_fmt("soccdpt_op_vit_attention_bwd", precision, &fmt)) return 1;
    if (th_vit_attention_bwd_mfma(dev_qkv, dev_attn_out, dev_dout, dev_rowstat, dev_dqkv, B, N, heads, (hipStream_t)stream, err, fmt))
        return fail(nullptr, "soccdpt_op_vit_attention_bwd: " + err);
    return 0;
}

int soccdpt_op_attn_param_grads(float* dev_ds, const float* dev_dscale_part, const float* dev_cpb_table, const float* dev_logit_scale, const float* dev_w0,
                                const float* dev_b0, const float* dev_w2, float* dev_dtable, float* dev_dt, float* dev_hid, float* dev_dls, float* dev_dw0,
                                float* dev_db0, float* dev_dw2, int nwin, int ws, int pws, int heads, void* stream) {
    std::string err;
    const char* who = "soccdpt_op_attn_param_grads: ";
    if (nwin <= 0 || ws <= 0 || heads <= 0 || pws < 0) return fail(nullptr, std::string(who) + "nwin, ws and heads must be positive, pws >= 0");
    const int slots = tr_attention_bwd_mfma_slots(ws);
    if (slots == 0) return fail(nullptr, std::string(who) + "no attention backward is instantiated for this window size");
    if (pws == 1 || (pws == 0 && ws == 1)) return fail(nullptr, std::string(who) + "the coordinates divide by the (pretrained) window size - 1");
    if (!dev_dls && !dev_dw0 && !dev_db0 && !dev_dw2) return fail(nullptr, std::string(who) + "no output requested");
    if (dev_dls && (!dev_dscale_part || !dev_logit_scale)) return fail(nullptr, std::string(who) + "dls needs dscale_part and logit_scale");
    if ((dev_dw0 || dev_db0 || dev_dw2) && (!dev_ds || !dev_cpb_table || !dev_w0 || !dev_b0 || !dev_w2 || !dev_dtable || !dev_dt || !dev_hid))
        return fail(nullptr, std::string(who) + "the table gradients need dS, the table, w0, b0, w2 and the dtable / dt / hid scratch");
    if (tr_attn_param_grads(dev_ds, dev_dscale_part, dev_cpb_table, dev_logit_scale, dev_w0, dev_b0, dev_w2, dev_dtable, dev_dt, dev_hid, dev_dls, dev_dw0, dev_db0,
                            dev_dw2, nwin, ws, pws, heads, slots, (hipStream_t)stream, err))
        return fail(nullptr, who + err);
    return 0;
}

int soccdpt_op_qv_bias_grad(const float* dev_dqkv_bias, float* dev_dq, float* dev_dv, int C, void* stream) {
    std::string err;
    if (!dev_dqkv_bias || (!dev_dq && !dev_dv)) return fail(nullptr, "soccdpt_op_qv_bias_grad: null argument (the input and at least one output)");
    if (C <= 0) return fail(nullptr, "soccdpt_op_qv_bias_grad: C must be positive");
    if (tr_qv_bias_grad(dev_dqkv_bias, dev_dq, dev_dv, C, (hipStream_t)stream, err)) return fail(nullptr, "soccdpt_op_qv_bias_grad: " + err);
    return 0;
}

int soccdpt_op_vit_attention_out(const void* dev_qkv, void* dev_out, int precision, int out_x3, int B, int N, int heads, void* stream) {
    std::string err;
    if (!dev_qkv || !dev_out) return fail(nullptr, "soccdpt_op_vit_attention: null argument");
    if (precision != SOCCDPT_PREC_BF16 && precision != SOCCDPT_PREC_F32 && precision != SOCCDPT_PREC_F16 && precision != SOCCDPT_PREC_F16X3)
        return fail(nullptr, "soccdpt_op_vit_attention: unknown precision");
    if (out_x3 && precision != SOCCDPT_PREC_F16) return fail(nullptr, "soccdpt_op_vit_attention: the x3 output form belongs to the fp16 kernel");
    if (launch_vit_attention(dev_qkv, dev_out, precision, B, N, heads, (hipStream_t)stream, err, out_x3 ? 1 : 0)) return fail(nullptr, err);
    return 0;
}

int soccdpt_op_vit_attention(const void* dev_qkv, void* dev_out, int precision, int B, int N, int heads, void* stream) {
    return soccdpt_op_vit_attention_out(dev_qkv, dev_out, precision, 0, B, N, heads, stream);
}

int soccdpt_op_window_attention(const void* dev_qkv, const float* dev_cpb_table, const float* dev_scale, void* dev_out,
                                float* dev_bias_scratch, int B, int res, int ws, int shift, int heads, int precision, void* stream) {
    std::string err;
    if (precision != SOCCDPT_PREC_BF16 && precision != SOCCDPT_PREC_F32 && precision != SOCCDPT_PREC_F16 && precision != SOCCDPT_PREC_F16X3)
        return fail(nullptr, "soccdpt_op_window_attention: unknown precision");
    if (!dev_qkv || !dev_cpb_table || !dev_scale || !dev_out || !dev_bias_scratch) return fail(nullptr, "soccdpt_op_window_attention: null argument");
    if (window_attention_geometry("soccdpt_op_window_attention", B, res, ws, shift, heads, err)) return fail(nullptr, err);   // before the bias launch: nothing runs on a refusal
    if (precision == SOCCDPT_PREC_BF16 || precision == SOCCDPT_PREC_F16) {   // what launch_window_attention has no instantiation for, refused here as well: before the bias launch
        if (ws != 16 && ws != 8 && ws != 24 && ws != 12) return fail(nullptr, "soccdpt_op_window_attention: window size not instantiated (16, 8, 24, 12 are)");
        if (ws == 8 && shift != 0) return fail(nullptr, "soccdpt_op_window_attention: shifted 8x8 windows are not instantiated");
    }
    if (launch_attn_bias(dev_cpb_table, dev_bias_scratch, ws, heads, (hipStream_t)stream, err)) return fail(nullptr, err);
    if (precision == SOCCDPT_PREC_F32 || precision == SOCCDPT_PREC_F16X3) {   // F16X3: f32 qkv in, x3 operand out
        if (launch_window_attention_f32(static_cast<const float*>(dev_qkv), dev_bias_scratch, dev_cpb_table, dev_scale, static_cast<float*>(dev_out), B,
                                        res, ws, shift, heads, (hipStream_t)stream, err, precision == SOCCDPT_PREC_F16X3 ? 1 : 0))
            return fail(nullptr, err);
        return 0;
    }
    if (launch_window_attention(static_cast<const bf16_t*>(dev_qkv), dev_bias_scratch, dev_scale, static_cast<bf16_t*>(dev_out),
                                precision == SOCCDPT_PREC_F16 ? 1 : 0, B, res, ws, shift, heads, (hipStream_t)stream, err))
        return fail(nullptr, err);
    return 0;
}

int soccdpt_op_window_attention_qkv(const void* dev_x, const void* dev_wqkv, const float* dev_qkv_bias, const float* dev_cpb_table, const float* dev_scale,
                                    void* dev_out, float* dev_bias_scratch, int B, int res, int ws, int shift, int heads, int precision, int out_x3, void* dev_stamps, void* stream) {
    std::string err;
    if (!dev_x || !dev_wqkv || !dev_qkv_bias || !dev_cpb_table || !dev_scale || !dev_out || !dev_bias_scratch) return fail(nullptr, "soccdpt_op_window_attention_qkv: null argument");
    if (precision != SOCCDPT_PREC_BF16 && precision != SOCCDPT_PREC_F16 && precision != SOCCDPT_PREC_F16X2W)
        return fail(nullptr, "soccdpt_op_window_attention_qkv: precision is SOCCDPT_PREC_BF16, _F16 or _F16X2W (16-bit activations)");
    if (window_attention_geometry("soccdpt_op_window_attention_qkv", B, res, ws, shift, heads, err)) return fail(nullptr, err);   // before the bias launch
    if (ws == 8 && shift != 0) return fail(nullptr, "soccdpt_op_window_attention_qkv: shifted 8x8 windows are not instantiated");
    if (!window_attention_qkv_supported(ws, heads * 32, precision == SOCCDPT_PREC_F16X2W)) return fail(nullptr, "soccdpt_op_window_attention_qkv: window size / width not instantiated (16 x 16 and 8 x 8 windows)");
    if (launch_attn_bias(dev_cpb_table, dev_bias_scratch, ws, heads, (hipStream_t)stream, err)) return fail(nullptr, err);
    if (launch_window_attention_qkv(static_cast<const bf16_t*>(dev_x), dev_wqkv, dev_qkv_bias, dev_bias_scratch, dev_scale, static_cast<bf16_t*>(dev_out),
                                    precision != SOCCDPT_PREC_BF16 ? 1 : 0, precision == SOCCDPT_PREC_F16X2W ? 1 : 0, B, res, ws, shift, heads, (hipStream_t)stream, err, out_x3, static_cast<unsigned long long*>(dev_stamps)))
        return fail(nullptr, err);
    return 0;
}

int soccdpt_op_wino_weights(const float* dev_w, const float* dev_scale, void* dev_u, int N, int C, int precision, void* stream) {
    std::string err;
    if (!dev_w || !dev_u || (precision != SOCCDPT_PREC_BF16 && precision != SOCCDPT_PREC_F16)) return fail(nullptr, "soccdpt_op_wino_weights: null argument or precision not BF16 / F16");
    if (launch_wino_weights(dev_w, dev_scale, dev_u, precision == SOCCDPT_PREC_F16 ? 1 : 0, N, C, (hipStream_t)stream, err)) return fail(nullptr, err);
    return 0;
}
int soccdpt_op_wino_conv(const void* dev_x_halo, const void* dev_u, int B, int H, int W, int C, int N, const float* dev_bias, const float* dev_res1, const float* dev_res2,
                         int res2_h, int res2_w, int relu, int act_on_f32, float* dev_out_f32, void* dev_out_op, int out_halo, int out_x3, int precision, void* dev_stamps, void* stream) {
    std::string err;
    if (precision != SOCCDPT_PREC_BF16 && precision != SOCCDPT_PREC_F16) return fail(nullptr, "soccdpt_op_wino_conv: precision is SOCCDPT_PREC_BF16 or _F16");
    if (dev_res2 && (res2_h <= 0 || res2_w <= 0)) return fail(nullptr, "soccdpt_op_wino_conv: dev_res2 needs its source size (res2_h, res2_w > 0)");
    if (B <= 0) return fail(nullptr, "soccdpt_op_wino_conv: B must be positive");
    WinoArgs a;
    a.X = dev_x_halo; a.U = dev_u; a.B = B; a.H = H; a.W = W; a.C = C; a.N = N; a.bias = dev_bias; a.res1 = dev_res1; a.res2 = dev_res2; a.res2_h = res2_h; a.res2_w = res2_w;
    a.act = relu ? ACT_RELU : ACT_NONE; a.act_on_f32 = act_on_f32; a.out_f32 = dev_out_f32; a.out_op = dev_out_op; a.out_halo = out_halo; a.out_x3 = out_x3;
    a.hf = precision == SOCCDPT_PREC_F16 ? 1 : 0;
    a.stamps = static_cast<unsigned long long*>(dev_stamps);
    if (launch_wino_conv(a, (hipStream_t)stream, err)) return fail(nullptr, err);
    return 0;
}

int soccdpt_op_gn_finish(const float* dev_part, float* dev_stats, int B, int tps, int groups, int hw, int cpg, float eps, void* stream) {
    std::string err;
    if (launch_gn_finish(dev_part, dev_stats, B, tps, groups, hw, cpg, eps, (hipStream_t)stream, err)) return fail(nullptr, err);
    return 0;
}

// soccdpt_op_gn_apply (halo_format < 0: the halo image in out_format, GnApplyArgs::halo_mode = -1) and soccdpt_op_gn_apply_halo
static int op_gn_apply_impl(const char* who, const float* dev_raw, float* dev_stats, const float* dev_part, int tps, const float* dev_gamma, const float* dev_beta,
                            const float* dev_raw2, float* dev_stats2, const float* dev_part2, int tps2, const float* dev_gamma2, const float* dev_beta2,
                            const float* dev_res, float* dev_out_f32, void* dev_out_op, void* dev_out_halo, int out_format, int halo_format, int relu, size_t M,
                            int hw, int w, int C, int cpg, float eps, void* stream) {
    std::string err;
    if (!dev_raw || !dev_stats || !dev_gamma || !dev_beta || hw <= 0 || w <= 0 || hw % w) return fail(nullptr, std::string(who) + ": bad arguments");
    // the kernel reads these three whenever raw2 is there; the model always has them, a test entry has to ask
    if (dev_raw2 && (!dev_stats2 || !dev_gamma2 || !dev_beta2)) return fail(nullptr, std::string(who) + ": the projection shortcut needs stats2, gamma2 and beta2");
    auto mode_of = [](int f) { return f == SOCCDPT_PREC_BF16 ? 0 : (f == SOCCDPT_PREC_F16 ? 1 : (f == SOCCDPT_PREC_F32 ? 2 : (f == SOCCDPT_PREC_F16X3 ? 3 : -1))); };
    const int om = mode_of(out_format);
    if (om < 0) return fail(nullptr, std::string(who) + ": out_format is SOCCDPT_PREC_BF16, _F16, _F32 or _F16X3");
    const int hm = halo_format < 0 ? -1 : mode_of(halo_format);
    if (halo_format >= 0 && hm < 0) return fail(nullptr, std::string(who) + ": halo_format is SOCCDPT_PREC_BF16, _F16, _F32 or _F16X3");
    GnApplyArgs g;
    g.raw = dev_raw; g.stats = dev_stats; g.part = dev_part; g.tps = tps; g.gamma = dev_gamma; g.beta = dev_beta;
    g.raw2 = dev_raw2; g.stats2 = dev_stats2; g.part2 = dev_part2; g.tps2 = tps2; g.gamma2 = dev_gamma2; g.beta2 = dev_beta2; g.res = dev_res;
    g.out_f32 = dev_out_f32; g.out_op = dev_out_op; g.out_halo = dev_out_halo; g.halo_mode = hm; g.relu = relu; g.M = M; g.HW = hw; g.W = w; g.C = C; g.cpg = cpg; g.eps = eps;
    if (launch_gn_apply(g, om, (hipStream_t)stream, err)) return fail(nullptr, err);
    return 0;
}

int soccdpt_op_gn_apply(const float* dev_raw, float* dev_stats, const float* dev_part, int tps, const float* dev_gamma, const float* dev_beta,
                        const float* dev_raw2, float* dev_stats2, const float* dev_part2, int tps2, const float* dev_gamma2, const float* dev_beta2,
                        const float* dev_res, float* dev_out_f32, void* dev_out_op, void* dev_out_halo, int out_format, int relu, size_t M, int hw, int w,
                        int C, int cpg, float eps, void* stream) {
    return op_gn_apply_impl("soccdpt_op_gn_apply", dev_raw, dev_stats, dev_part, tps, dev_gamma, dev_beta, dev_raw2, dev_stats2, dev_part2, tps2, dev_gamma2, dev_beta2,
                            dev_res, dev_out_f32, dev_out_op, dev_out_halo, out_format, -1, relu, M, hw, w, C, cpg, eps, stream);
}

int soccdpt_op_gn_apply_halo(const float* dev_raw, float* dev_stats, const float* dev_part, int tps, const float* dev_gamma, const float* dev_beta,
                             const float* dev_raw2, float* dev_stats2, const float* dev_part2, int tps2, const float* dev_gamma2, const float* dev_beta2,
                             const float* dev_res, float* dev_out_f32, void* dev_out_op, void* dev_out_halo, int out_format, int halo_format, int relu, size_t M,
                             int hw, int w, int C, int cpg, float eps, void* stream) {
    if (halo_format < 0) return fail(nullptr, "soccdpt_op_gn_apply_halo: halo_format is SOCCDPT_PREC_BF16, _F16, _F32 or _F16X3");
    return op_gn_apply_impl("soccdpt_op_gn_apply_halo", dev_raw, dev_stats, dev_part, tps, dev_gamma, dev_beta, dev_raw2, dev_stats2, dev_part2, tps2, dev_gamma2,
                            dev_beta2, dev_res, dev_out_f32, dev_out_op, dev_out_halo, out_format, halo_format, relu, M, hw, w, C, cpg, eps, stream);
}

int soccdpt_workspace_tensor(void* handle, int B, const char* name, size_t* byte_offset, size_t* elems, int* kind, int* H, int* W,
                             int* C) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h || !name) return 1;
    return model_workspace_tensor(*h, B, name, byte_offset, elems, kind, H, W, C);
}

// ---- evaluation pictures (include/soccdpt_vis.h; csrc/visualise.hip) ----
size_t soccdpt_vis_minmax_scratch_bytes(int B, size_t npix) { return vis_minmax_scratch_bytes(B, npix); }

int soccdpt_vis_minmax(const float* dev_x, int B, size_t npix, float* dev_minmax, void* dev_scratch, size_t scratch_bytes, void* stream) {
    std::string err;
    if (launch_vis_minmax(dev_x, B, npix, dev_minmax, dev_scratch, scratch_bytes, (hipStream_t)stream, err)) return fail(nullptr, "soccdpt_" + err);
    return 0;
}

int soccdpt_vis_colorize(const float* dev_x, const float* dev_minmax, const uint8_t* dev_lut, int B, int H, int W, uint8_t* dev_dst,
                         size_t dst_pitch_px, size_t dst_offset_px, size_t dst_frame_px, size_t dst_total_px, void* stream) {
    std::string err;
    const VisDst d{dst_pitch_px, dst_offset_px, dst_frame_px, dst_total_px};
    if (launch_vis_colorize(dev_x, dev_minmax, dev_lut, B, H, W, dev_dst, d, (hipStream_t)stream, err)) return fail(nullptr, "soccdpt_" + err);
    return 0;
}

int soccdpt_vis_color_masks(const float* dev_seg, int B, int C, int H, int W, int channels_last, const uint8_t* dev_class_colors, uint8_t* dev_dst,
                            size_t dst_pitch_px, size_t dst_offset_px, size_t dst_frame_px, size_t dst_total_px, void* stream) {
    std::string err;
    const VisDst d{dst_pitch_px, dst_offset_px, dst_frame_px, dst_total_px};
    if (launch_vis_color_masks(dev_seg, B, C, H, W, channels_last, dev_class_colors, dev_dst, d, (hipStream_t)stream, err))
        return fail(nullptr, "soccdpt_" + err);
    return 0;
}

int soccdpt_vis_resize_taps(int src, int dst, int32_t* host_taps) {
    std::string err;
    if (vis_resize_taps(src, dst, host_taps, err)) return fail(nullptr, "soccdpt_" + err);
    return 0;
}

int soccdpt_vis_resize(const uint8_t* dev_src, int B, int Hs, int Ws, const int32_t* dev_ytaps, const int32_t* dev_xtaps, int Hd, int Wd,
                       uint8_t* dev_dst, size_t dst_pitch_px, size_t dst_offset_px, size_t dst_frame_px, size_t dst_total_px, void* stream) {
    std::string err;
    const VisDst d{dst_pitch_px, dst_offset_px, dst_frame_px, dst_total_px};
    if (launch_vis_resize(dev_src, B, Hs, Ws, dev_ytaps, dev_xtaps, Hd, Wd, dev_dst, d, (hipStream_t)stream, err)) return fail(nullptr, "soccdpt_" + err);
    return 0;
}

int soccdpt_vis_half_size(int H, int W, int32_t* Hd, int32_t* Wd) {
    if (!Hd || !Wd || H < 2 || W < 2) return fail(nullptr, "soccdpt_vis_half_size: null argument, or H or W below 2");
    int h, w;
    vis_half_size(H, W, &h, &w);
    *Hd = h;
    *Wd = w;
    return 0;
}

int soccdpt_vis_shrink_half(const uint8_t* dev_src, int B, int H, int W, int swap_rb, uint8_t* dev_dst, void* stream) {
    std::string err;
    if (launch_vis_shrink_half(dev_src, B, H, W, swap_rb, dev_dst, (hipStream_t)stream, err)) return fail(nullptr, "soccdpt_" + err);
    return 0;
}

// ---- occupancy grid pictures (include/soccdpt_occ_view.h; csrc/occ_view.hip) ----
int soccdpt_occ_view_columns(const uint32_t* dev_bits, int rows, const int32_t* host_grid, int C, int axis, int from_high, uint8_t* dev_top,
                             int32_t* dev_first, int32_t* dev_count, uint8_t* dev_classes, void* stream) {
    std::string err;
    if (launch_occ_view_columns(dev_bits, rows, host_grid, C, axis, from_high, dev_top, dev_first, dev_count, dev_classes, (hipStream_t)stream, err))
        return fail(nullptr, "soccdpt_" + err);
    return 0;
}

int soccdpt_occ_view_paint(const uint8_t* dev_top, const int32_t* dev_first, int rows, int A, int B, int depth_len, int from_high,
                           const uint8_t* dev_class_colors, int C, const uint8_t* host_background, int shade, int zoom, int flip_a, int flip_b,
                           int transpose, uint8_t* dev_dst, size_t dst_pitch_px, size_t dst_offset_px, size_t dst_frame_px, size_t dst_total_px,
                           void* stream) {
    std::string err;
    const VisDst d{dst_pitch_px, dst_offset_px, dst_frame_px, dst_total_px};
    if (launch_occ_view_paint(dev_top, dev_first, rows, A, B, depth_len, from_high, dev_class_colors, C, host_background, shade, zoom, flip_a, flip_b,
                              transpose, dev_dst, d, (hipStream_t)stream, err))
        return fail(nullptr, "soccdpt_" + err);
    return 0;
}

int soccdpt_occ_view_iou2d(const uint8_t* dev_pred_classes, int pred_rows, const uint8_t* dev_gt_classes, int rows, size_t ncol, int C,
                           uint64_t* dev_counts, void* stream) {
    std::string err;
    if (launch_occ_view_iou2d(dev_pred_classes, pred_rows, dev_gt_classes, rows, ncol, C, dev_counts, (hipStream_t)stream, err))
        return fail(nullptr, "soccdpt_" + err);
    return 0;
}

int soccdpt_occ_view_splat(const uint32_t* dev_bits, int rows, const int32_t* host_grid, int C, const double* host_voxel_to_camera,
                           const double* host_intrinsics, double half_extent_m, int max_radius_px, double z_near, int H, int W, uint64_t* dev_zbuf,
                           void* stream) {
    std::string err;
    if (launch_occ_view_splat(dev_bits, rows, host_grid, C, host_voxel_to_camera, host_intrinsics, half_extent_m, max_radius_px, z_near, H, W, dev_zbuf,
                              (hipStream_t)stream, err))
        return fail(nullptr, "soccdpt_" + err);
    return 0;
}

int soccdpt_occ_view_resolve(const uint64_t* dev_zbuf, const uint8_t* dev_frames, int frame_rows, int rows, int H, int W, int C,
                             const uint8_t* dev_class_colors, int alpha, uint8_t* dev_dst, size_t dst_pitch_px, size_t dst_offset_px,
                             size_t dst_frame_px, size_t dst_total_px, void* stream) {
    std::string err;
    const VisDst d{dst_pitch_px, dst_offset_px, dst_frame_px, dst_total_px};
    if (launch_occ_view_resolve(dev_zbuf, dev_frames, frame_rows, rows, H, W, C, dev_class_colors, alpha, dev_dst, d, (hipStream_t)stream, err))
        return fail(nullptr, "soccdpt_" + err);
    return 0;
}

// ---- observed space by ray casting, and the 3-D IoU over it (include/soccdpt_occ_rays.h; csrc/occ_rays.hip) ----
int soccdpt_occ_rays_observed(const float* dev_depth, int rows, int H, int W, const int32_t* host_grid, const double* host_camera_to_voxel,
                              const double* host_intrinsics, double z_near, double max_depth, int step, int clear, uint32_t* dev_mask, void* stream) {
    std::string err;
    if (launch_occ_rays_observed(dev_depth, rows, H, W, host_grid, host_camera_to_voxel, host_intrinsics, z_near, max_depth, step, clear, dev_mask,
                                 (hipStream_t)stream, err))
        return fail(nullptr, "soccdpt_" + err);
    return 0;
}

int soccdpt_occ_iou_counts_masked(const uint32_t* dev_pred_bits, int pred_rows, const uint32_t* dev_gt_bits, int rows, size_t nvox, int C,
                                  const uint32_t* dev_mask, int mask_rows, int include_gt, uint64_t* dev_counts, uint64_t* dev_observed,
                                  void* stream) {
    std::string err;
    if (launch_occ_iou_counts_masked(dev_pred_bits, pred_rows, dev_gt_bits, rows, nvox, C, dev_mask, mask_rows, include_gt, dev_counts, dev_observed,
                                     (hipStream_t)stream, err))
        return fail(nullptr, "soccdpt_" + err);
    return 0;
}

// ---- batch targets (include/soccdpt_data.h; csrc/batch_targets.hip) ----
int soccdpt_data_targets(const uint8_t* dev_seg, const uint8_t* dev_colors, int C, const void* dev_disp, int disp_dtype, int B, int H, int W, int flip,
                         float* dev_onehot, int32_t* dev_class_map, float* dev_y_disp, uint64_t* dev_unmatched, void* stream) {
    std::string err;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the unmatched counters are 64-bit");
    if (launch_data_targets(dev_seg, dev_colors, C, dev_disp, disp_dtype, B, H, W, flip, dev_onehot, dev_class_map, dev_y_disp,
                            reinterpret_cast<unsigned long long*>(dev_unmatched), (hipStream_t)stream, err))
        return fail(nullptr, "soccdpt_" + err);
    return 0;
}

int soccdpt_data_resize_u8c1(const uint8_t* dev_src, int B, int Hs, int Ws, const int32_t* dev_ytaps, const int32_t* dev_xtaps, int Hd, int Wd,
                             uint8_t* dev_dst, void* stream) {
    std::string err;
    if (launch_data_resize_u8c1(dev_src, B, Hs, Ws, dev_ytaps, dev_xtaps, Hd, Wd, dev_dst, (hipStream_t)stream, err)) return fail(nullptr, "soccdpt_" + err);
    return 0;
}

}  // extern "C"
