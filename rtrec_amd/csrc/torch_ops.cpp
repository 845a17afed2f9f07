// rtrec_amd/csrc/torch_ops.cpp -- the PyTorch-ROCm custom ops `torch.ops.rtrec_amd.*`, registered from C++.
//
// One op per entry point of include/rtrec_amd.h (and of the extension surface, include/rtrec_amd_ext.h), in out-variant style: every buffer is a ROCm tensor owned by the
// caller, outputs and scratch are marked mutable in the schema, scalars are plain ints / floats / bools, and the work is
// enqueued on the current HIP stream of the tensors' device.  The ops only marshal pointers -- all computation is in
// librtrec_amd.so, which this library binds at run time (rtrec_ops_bind: dlopen + dlsym of the C-ABI, so an A/B build
// of the kernels can be selected with RTREC_AMD_LIB like before) -- so they compose with torch streams, the caching
// allocator and torch.distributed without copies.  Round 2 registered the same schemas from Python
// (torch.library.custom_op bodies that called ctypes); a call now goes dispatcher -> this function -> C-ABI.
//
// Built by rtrec_amd/build.py with the host compiler against the torch headers (no device code here).
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <c10/util/Optional.h>
#include <torch/library.h>

#include <dlfcn.h>

#include <stdexcept>
#include <string>
#include <vector>
#include <type_traits>

#include "../../include/rtrec_amd.h"
#include "../../include/rtrec_amd_ext.h"

namespace {

struct Abi {
    void *handle = nullptr;
    decltype(&rtrec_amd_last_error) last_error = nullptr;
    decltype(&rtrec_slim_column_sqnorms) column_sqnorms = nullptr;
    decltype(&rtrec_slim_fit_workspace_init) fit_workspace_init = nullptr;
    decltype(&rtrec_slim_gram_matrix) gram_matrix = nullptr;
    decltype(&rtrec_slim_fit_columns_opt) fit_columns_opt = nullptr;
    decltype(&rtrec_slim_score_topk_opt) score_topk_opt = nullptr;
    decltype(&rtrec_slim_score_rows) score_rows = nullptr;
    decltype(&rtrec_slim_merge_topk_strided) merge_topk_strided = nullptr;
    decltype(&rtrec_slim_similar_topk) similar_topk = nullptr;
    decltype(&rtrec_store_decay_device) store_decay_device = nullptr;
    decltype(&rtrec_store_fold_device) store_fold_device = nullptr;
    decltype(&rtrec_slim_fit_sgd_epochs) fit_sgd_epochs = nullptr;
    decltype(&rtrec_slim_first_touch_aux) first_touch_aux = nullptr;
    decltype(&rtrec_slim_dense_fill) dense_fill = nullptr;
    decltype(&rtrec_slim_refine_topk_f64) refine_topk_f64 = nullptr;
    decltype(&rtrec_slim_score_candidates) score_candidates = nullptr;
    decltype(&rtrec_slim_seg_plan) seg_plan = nullptr;
    decltype(&rtrec_slim_seg_fill) seg_fill = nullptr;
    decltype(&rtrec_slim_ordered_sums) ordered_sums = nullptr;
    decltype(&rtrec_rank_metrics) rank_metrics = nullptr;
    decltype(&rtrec_slim_explain_topk) explain_topk = nullptr;
    decltype(&rtrec_slim_audience_topk) audience_topk = nullptr;
    decltype(&rtrec_slim_score_pairs) score_pairs = nullptr;
    decltype(&rtrec_slim_diversify_lists) diversify_lists = nullptr;          // include/rtrec_amd_ext.h
    decltype(&rtrec_slim_list_quality) list_quality = nullptr;
    decltype(&rtrec_slim_catalogue_ranks) catalogue_ranks = nullptr;
    decltype(&rtrec_slim_blend_lists) blend_lists = nullptr;
    decltype(&rtrec_factor_topk) factor_topk = nullptr;
    decltype(&rtrec_feature_repr) feature_repr = nullptr;
    decltype(&rtrec_factor_norms) factor_norms = nullptr;
    decltype(&rtrec_factor_similar_topk) factor_similar_topk = nullptr;
    decltype(&rtrec_similar_blend) similar_blend = nullptr;
    decltype(&rtrec_factor_gram) factor_gram = nullptr;
    decltype(&rtrec_factor_als_solve) factor_als_solve = nullptr;
    decltype(&rtrec_factor_gram_wide) factor_gram_wide = nullptr;
    decltype(&rtrec_factor_als_cg) factor_als_cg = nullptr;
};
Abi g_abi;

template <typename F>
void bind_one(void *h, F &slot, const char *name) {
    slot = reinterpret_cast<F>(dlsym(h, name));
    if (!slot) throw std::runtime_error(std::string("librtrec_amd.so does not export ") + name);
}

const Abi &abi() {
    TORCH_CHECK(g_abi.handle, "rtrec_amd ops are not bound to librtrec_amd.so (rtrec_amd.ops binds them at import)");
    return g_abi;
}

void check(int status, const char *what) {
    if (status == 0) return;
    const char *names[] = {"ok", "invalid argument", "unsupported parameter", "workspace too small", "kernel launch failed"};
    const int k = -status;
    std::string msg = std::string(what) + " failed: " + (k >= 0 && k <= 4 ? names[k] : "error") + " (" + std::to_string(status) + ")";
    if (status == -4 && g_abi.last_error) msg += std::string(" ") + g_abi.last_error();
    TORCH_CHECK(false, msg);
}

// The C-ABI takes raw device pointers: a tensor of another dtype, a strided view or a host tensor in any slot would be a
// silent out-of-bounds access on the GPU, so every pointer handed over is checked against the element type its slot
// declares.  ptr<void> / ptr<unsigned char> slots are byte workspaces: any dtype, still contiguous + device.
template <typename T> struct ElemOf { static bool ok(at::ScalarType) { return true; } };
template <> struct ElemOf<int32_t> { static bool ok(at::ScalarType s) { return s == at::kInt; } };
template <> struct ElemOf<uint32_t> { static bool ok(at::ScalarType s) { return s == at::kInt || s == at::kUInt32; } };
template <> struct ElemOf<int64_t> { static bool ok(at::ScalarType s) { return s == at::kLong; } };
template <> struct ElemOf<float> { static bool ok(at::ScalarType s) { return s == at::kFloat; } };
template <> struct ElemOf<double> { static bool ok(at::ScalarType s) { return s == at::kDouble; } };

template <typename T>
void check_tensor(const at::Tensor &t) {
    TORCH_CHECK(t.is_contiguous(), "rtrec_amd op: tensor argument must be contiguous (got strides of a view)");
    TORCH_CHECK(t.device().is_cuda(), "rtrec_amd op: tensor argument must live on the GPU, got ", t.device());
    TORCH_CHECK(ElemOf<typename std::remove_const<T>::type>::ok(t.scalar_type()), "rtrec_amd op: tensor argument has dtype ",
                t.scalar_type(), ", the slot takes ", sizeof(T) == 8 ? "a 64-bit" : "a 32-bit", " element type");
}
template <> void check_tensor<void>(const at::Tensor &t) {
    TORCH_CHECK(t.is_contiguous() && t.device().is_cuda(), "rtrec_amd op: workspace tensors must be contiguous GPU tensors");
}
template <> void check_tensor<const void>(const at::Tensor &t) { check_tensor<void>(t); }

// strided inputs (merge_topk: views of an exchanged record buffer, their strides travel as arguments): dtype + device only
template <typename T>
T *sptr(const at::Tensor &t) {
    if (t.numel() == 0) return nullptr;
    TORCH_CHECK(t.device().is_cuda(), "rtrec_amd op: tensor argument must live on the GPU, got ", t.device());
    TORCH_CHECK(ElemOf<typename std::remove_const<T>::type>::ok(t.scalar_type()), "rtrec_amd op: tensor argument has dtype ", t.scalar_type());
    return static_cast<T *>(t.data_ptr());
}
template <typename T>
T *sptr(const c10::optional<at::Tensor> &t) { return (t.has_value() && t->defined()) ? sptr<T>(*t) : nullptr; }

template <typename T = void>
T *ptr(const at::Tensor &t) {
    if (t.numel() == 0) return nullptr;
    check_tensor<T>(t);
    return static_cast<T *>(t.data_ptr());
}
template <typename T = void>
T *ptr(const c10::optional<at::Tensor> &t) {
    if (!(t.has_value() && t->defined() && t->numel() > 0)) return nullptr;
    check_tensor<T>(*t);
    return static_cast<T *>(t->data_ptr());
}

void *stream_of(const at::Tensor &t) {
    return static_cast<void *>(c10::hip::getCurrentHIPStream(t.device().index()).stream());
}

using OT = c10::optional<at::Tensor>;

void column_sqnorms(const at::Tensor &cptr, const at::Tensor &cval, at::Tensor out) {
    check(abi().column_sqnorms(static_cast<int32_t>(out.size(0)), ptr<const int32_t>(cptr), ptr<const float>(cval), ptr<float>(out),
                               stream_of(out)), "rtrec_slim_column_sqnorms");
}

void fit_workspace_init(at::Tensor ws, int64_t n_users, int64_t n_items, int64_t n_slots, int64_t top_features) {
    check(abi().fit_workspace_init(ptr(ws), static_cast<size_t>(ws.numel()), n_users, n_items, n_slots, top_features, stream_of(ws)),
          "rtrec_slim_fit_workspace_init");
}

void gram_matrix(const at::Tensor &cptr, const at::Tensor &crow, const at::Tensor &cval, const at::Tensor &top_items, at::Tensor ws,
                 at::Tensor gram, int64_t n_users, int64_t n_items) {
    check(abi().gram_matrix(n_users, n_items, ptr<const int32_t>(cptr), ptr<const int32_t>(crow), ptr<const float>(cval),
                            ptr<const int32_t>(top_items), static_cast<int32_t>(top_items.size(0)), ptr(ws),
                            static_cast<size_t>(ws.numel()), ptr<double>(gram), stream_of(gram)), "rtrec_slim_gram_matrix");
}

void fit_columns(const at::Tensor &cptr, const at::Tensor &crow, const at::Tensor &cval, const at::Tensor &rptr, const at::Tensor &rcol,
                 const at::Tensor &rval, const at::Tensor &sqn, const at::Tensor &targets, int64_t n_users, int64_t n_items,
                 double l1_reg, double l2_reg, double tol, int64_t max_iter, int64_t seed, bool positive, int64_t top_features,
                 at::Tensor out_items, at::Tensor out_coef, at::Tensor out_count, at::Tensor out_n_iter, int64_t cap, at::Tensor ws,
                 int64_t n_slots, at::Tensor queue, OT trace, const OT &gram, const OT &gram_index, int64_t gram_n, double gram_rel_err,
                 int64_t fast, int64_t kernel, int64_t colwalk_min_rows, int64_t screen_min, int64_t lane_max, OT xty_ws,
                 const OT &col_order, int64_t fold) {
    rtrec_fit_cfg cfg{static_cast<float>(l1_reg), static_cast<float>(l2_reg), static_cast<float>(tol), static_cast<int32_t>(max_iter),
                      static_cast<uint32_t>(seed), positive ? 1 : 0, static_cast<int32_t>(top_features)};
    rtrec_fit_opts o{};
    o.d_trace = ptr<int64_t>(trace);
    o.d_gram = ptr<const double>(gram);
    o.d_gram_index = ptr<const int32_t>(gram_index);
    o.gram_n = o.d_gram ? static_cast<int32_t>(gram_n) : 0;
    o.gram_rel_err = gram_rel_err;
    o.fast = static_cast<int32_t>(fast);
    o.kernel = static_cast<int32_t>(kernel);
    o.colwalk_min_rows = static_cast<int32_t>(colwalk_min_rows);
    o.screen_min = static_cast<int32_t>(screen_min);
    o.lane_max = static_cast<int32_t>(lane_max);
    o.d_xty_ws = ptr(xty_ws);
    o.xty_ws_bytes = (xty_ws.has_value() && xty_ws->defined()) ? static_cast<size_t>(xty_ws->numel()) : 0;
    o.nnz = rcol.size(0);
    o.d_col_order = ptr<const int32_t>(col_order);
    o.fold = static_cast<int32_t>(fold);
    check(abi().fit_columns_opt(n_users, n_items, ptr<const int32_t>(cptr), ptr<const int32_t>(crow), ptr<const float>(cval),
                                ptr<const int32_t>(rptr), ptr<const int32_t>(rcol), ptr<const float>(rval), ptr<const float>(sqn),
                                ptr<const int32_t>(targets), static_cast<int32_t>(targets.size(0)), &cfg, ptr<int32_t>(out_items),
                                ptr<float>(out_coef), ptr<int32_t>(out_count), ptr<int32_t>(out_n_iter), static_cast<int32_t>(cap), ptr(ws),
                                static_cast<size_t>(ws.numel()), static_cast<int32_t>(n_slots), ptr<int32_t>(queue), stream_of(out_items), &o),
          "rtrec_slim_fit_columns_opt");
}

void score_topk(const OT &row_ids, const at::Tensor &xb_ptr, const at::Tensor &xb_col, const at::Tensor &xb_val, int64_t n_rows,
                int64_t n_items, int64_t n_cols, int64_t col_offset, const OT &col_ids, const OT &col_map, int64_t tile_cols,
                int64_t n_tiles, const OT &tile_ptr, const OT &w_col, const OT &w_val, const OT &dense_idx, const OT &dense_val,
                const OT &row_hdr, const OT &col_rank, int64_t top_k, bool filter_interacted, int64_t mode, bool acc_f64, at::Tensor ids,
                at::Tensor scores, OT scores64, at::Tensor aux, at::Tensor count, at::Tensor ws, const OT &fr_map, const OT &fr_col_ids,
                const OT &fr_col_map, const OT &fr_w, const OT &fr_tile_rows, const OT &fr_tile_off, const OT &fr_super_kb,
                const OT &fr_super_tile, const OT &fr_frag_tile, int64_t fr_rows, int64_t fr_tile_cols, int64_t fr_n_tiles,
                int64_t fr_n_frags, int64_t fr_n_super, int64_t fr_buf_bytes, OT fr_scratch, const OT &row_order, int64_t timer,
                int64_t diagnostics, OT rescored, int64_t row_order_grouped, const OT &sg_info, const OT &sg_ptr, const OT &sg_ent,
                const OT &sg_bound, const OT &sg_col_ids, int64_t sg_tile_cols, int64_t sg_n_tiles, int64_t sg_rows, int64_t sg_n_cols,
                const OT &sg_trow_ptr, const OT &sg_trow, OT sg_scratch, OT flagged, int64_t aux_stream) {
    rtrec_score_opts o{};
    o.n_x_rows = static_cast<int32_t>(xb_ptr.size(0)) - 1;
    o.d_fr_map = ptr<const int32_t>(fr_map);
    o.d_fr_col_ids = ptr<const int32_t>(fr_col_ids);
    o.d_fr_col_map = ptr<const int32_t>(fr_col_map);
    o.d_fr_w = ptr<const float>(fr_w);
    o.d_fr_tile_rows = ptr<const uint64_t>(fr_tile_rows);
    o.d_fr_tile_off = ptr<const int32_t>(fr_tile_off);
    o.d_fr_super_kb = ptr<const int32_t>(fr_super_kb);
    o.d_fr_super_tile = ptr<const int32_t>(fr_super_tile);
    o.d_fr_frag_tile = ptr<const int32_t>(fr_frag_tile);
    o.fr_rows = static_cast<int32_t>(fr_rows); o.fr_tile_cols = static_cast<int32_t>(fr_tile_cols);
    o.fr_n_tiles = static_cast<int32_t>(fr_n_tiles); o.fr_n_frags = static_cast<int32_t>(fr_n_frags);
    o.fr_n_super = static_cast<int32_t>(fr_n_super); o.fr_buf_bytes = static_cast<int32_t>(fr_buf_bytes);
    o.d_fr_scratch = ptr(fr_scratch);
    o.fr_scratch_bytes = (fr_scratch.has_value() && fr_scratch->defined()) ? static_cast<size_t>(fr_scratch->numel()) : 0;
    o.d_row_order = ptr<const int32_t>(row_order);
    o.timer = reinterpret_cast<void *>(static_cast<intptr_t>(timer));
    o.diagnostics = static_cast<int32_t>(diagnostics);
    o.d_rescored = ptr<int32_t>(rescored);
    o.row_order_grouped = static_cast<int32_t>(row_order_grouped & 1);      // the schema holds 64 arguments at most: two flags in one
    o.row_order_longest_first = static_cast<int32_t>((row_order_grouped >> 1) & 1);
    o.d_sg_info = ptr<const int32_t>(sg_info);
    o.d_sg_ptr = ptr<const int32_t>(sg_ptr);
    o.d_sg_ent = ptr<const uint32_t>(sg_ent);
    o.sg_nnz = (sg_ent.has_value() && sg_ent->defined()) ? sg_ent->size(0) : 0;
    o.d_sg_bound = ptr<const uint32_t>(sg_bound);
    o.d_sg_col_ids = ptr<const int32_t>(sg_col_ids);
    o.sg_tile_cols = static_cast<int32_t>(sg_tile_cols); o.sg_n_tiles = static_cast<int32_t>(sg_n_tiles);
    o.sg_rows = static_cast<int32_t>(sg_rows); o.sg_n_cols = static_cast<int32_t>(sg_n_cols);
    o.d_sg_trow_ptr = ptr<const int32_t>(sg_trow_ptr);
    o.d_sg_trow = ptr<const int32_t>(sg_trow);
    o.d_sg_scratch = ptr(sg_scratch);
    o.sg_scratch_bytes = (sg_scratch.has_value() && sg_scratch->defined()) ? static_cast<size_t>(sg_scratch->numel()) : 0;
    o.d_flagged = ptr<int32_t>(flagged);
    o.aux_stream = reinterpret_cast<void *>(static_cast<intptr_t>(aux_stream));
    check(abi().score_topk_opt(static_cast<int32_t>(n_rows), ptr<const int32_t>(row_ids), ptr<const int32_t>(xb_ptr),
                               ptr<const int32_t>(xb_col), ptr<const float>(xb_val), static_cast<int32_t>(n_items),
                               static_cast<int32_t>(n_cols), static_cast<int32_t>(col_offset), ptr<const int32_t>(col_ids),
                               ptr<const int32_t>(col_map), static_cast<int32_t>(tile_cols), static_cast<int32_t>(n_tiles),
                               ptr<const int32_t>(tile_ptr), ptr<const uint16_t>(w_col), ptr<const float>(w_val),
                               ptr<const int32_t>(dense_idx), ptr<const float>(dense_val), ptr<const int32_t>(row_hdr),
                               ptr<const int32_t>(col_rank), static_cast<int32_t>(top_k), filter_interacted ? 1 : 0,
                               static_cast<int32_t>(mode), acc_f64 ? 1 : 0, ptr<int32_t>(ids), ptr<float>(scores), ptr<double>(scores64),
                               ptr<uint32_t>(aux), ptr<int32_t>(count), ptr(ws), static_cast<size_t>(ws.numel()), stream_of(ids), &o),
          "rtrec_slim_score_topk_opt");
}

void score_rows(const OT &row_ids, const at::Tensor &xb_ptr, const at::Tensor &xb_col, const at::Tensor &xb_val, int64_t n_rows,
                int64_t n_items, int64_t n_cols, int64_t col_offset, int64_t tile_cols, int64_t n_tiles, const at::Tensor &tile_ptr,
                const at::Tensor &w_col, const at::Tensor &w_val, bool acc_f64, at::Tensor out) {
    check(abi().score_rows(static_cast<int32_t>(n_rows), ptr<const int32_t>(row_ids), ptr<const int32_t>(xb_ptr), ptr<const int32_t>(xb_col),
                           ptr<const float>(xb_val), static_cast<int32_t>(n_items), static_cast<int32_t>(n_cols),
                           static_cast<int32_t>(col_offset), static_cast<int32_t>(tile_cols), static_cast<int32_t>(n_tiles),
                           ptr<const int32_t>(tile_ptr), ptr<const uint16_t>(w_col), ptr<const float>(w_val), acc_f64 ? 1 : 0, ptr(out),
                           out.stride(0), stream_of(out)), "rtrec_slim_score_rows");
}

// in_* are [n_lists, n_rows, top_k] (in_count [n_lists, n_rows]); strided views into one packed all-gather buffer are
// fine as long as the last dimension is contiguous.
void merge_topk(const at::Tensor &in_ids, const at::Tensor &in_scores, const OT &in_scores64, const at::Tensor &in_aux,
                const at::Tensor &in_count, int64_t top_k, at::Tensor out_ids, at::Tensor out_scores, at::Tensor out_count) {
    TORCH_CHECK(in_ids.dim() == 3 && in_ids.stride(2) == 1 && in_ids.strides() == in_scores.strides() &&
                in_ids.strides() == in_aux.strides(), "merge_topk: ids / scores / aux must share strides, last dimension contiguous");
    int64_t s64_0 = 0, s64_1 = 0;
    if (in_scores64.has_value() && in_scores64->defined()) {
        TORCH_CHECK(in_scores64->stride(2) == 1, "merge_topk: scores64 last dimension must be contiguous");
        s64_0 = in_scores64->stride(0); s64_1 = in_scores64->stride(1);
    }
    check(abi().merge_topk_strided(static_cast<int32_t>(in_ids.size(1)), static_cast<int32_t>(in_ids.size(0)), static_cast<int32_t>(top_k),
                                   sptr<const int32_t>(in_ids), sptr<const float>(in_scores), sptr<const double>(in_scores64),
                                   sptr<const uint32_t>(in_aux), sptr<const int32_t>(in_count), in_ids.stride(0), in_ids.stride(1), s64_0,
                                   s64_1, in_count.stride(0), in_count.stride(1), ptr<int32_t>(out_ids), ptr<float>(out_scores),
                                   ptr<int32_t>(out_count), stream_of(out_ids)), "rtrec_slim_merge_topk_strided");
}

void similar_topk(const at::Tensor &queries, const at::Tensor &wc_ptr, const at::Tensor &wc_row, const at::Tensor &wc_val, int64_t top_k,
                  at::Tensor ids, at::Tensor scores, at::Tensor count) {
    check(abi().similar_topk(static_cast<int32_t>(queries.size(0)), ptr<const int32_t>(queries), ptr<const int32_t>(wc_ptr),
                             ptr<const int32_t>(wc_row), ptr<const float>(wc_val), static_cast<int32_t>(top_k), ptr<int32_t>(ids),
                             ptr<float>(scores), ptr<int32_t>(count), stream_of(ids)), "rtrec_slim_similar_topk");
}

// ---- round 5: the device entry points that used to be called by raw ctypes, same typed checks ----
void store_decay_device(const at::Tensor &raw, const at::Tensor &ts, double rate, double now, at::Tensor out, at::Tensor unsafe_idx,
                        at::Tensor unsafe_count) {
    TORCH_CHECK(ts.numel() == raw.numel() && out.numel() == raw.numel(), "store_decay_device: raw, ts and out must have one length");
    check(abi().store_decay_device(ptr<const double>(raw), ptr<const double>(ts), raw.numel(), rate, now, ptr<float>(out),
                                   ptr<int32_t>(unsafe_idx), ptr<int32_t>(unsafe_count), static_cast<int32_t>(unsafe_idx.numel()),
                                   stream_of(out)), "rtrec_store_decay_device");
}

void store_fold_device(const at::Tensor &order, const at::Tensor &start, const at::Tensor &delta, const at::Tensor &tstamp, const OT &old,
                       double lo, double hi, bool upsert, at::Tensor out_val, at::Tensor out_ts, at::Tensor out_val32) {
    const int64_t g = start.numel() - 1;
    TORCH_CHECK(g >= 0 && out_val.numel() == g && out_ts.numel() == g && out_val32.numel() == g, "store_fold_device: outputs must hold one entry per group");
    TORCH_CHECK(delta.numel() == order.numel() && tstamp.numel() == order.numel(), "store_fold_device: order, delta and tstamp must have one length");
    check(abi().store_fold_device(ptr<const int64_t>(order), ptr<const int64_t>(start), g, ptr<const double>(delta), ptr<const double>(tstamp),
                                  ptr<const double>(old), lo, hi, upsert ? 1 : 0, ptr<double>(out_val), ptr<double>(out_ts),
                                  ptr<float>(out_val32), stream_of(out_val)), "rtrec_store_fold_device");
}

void fit_sgd_epochs(const at::Tensor &cptr, const at::Tensor &ttime, const at::Tensor &tval, const at::Tensor &targets, const at::Tensor &sel,
                    const at::Tensor &sel_count, int64_t n_users, int64_t n_items, int64_t nnz, int64_t cap, int64_t first_epoch,
                    int64_t n_epochs, int64_t max_iter, double tol, const at::Tensor &eta, const at::Tensor &ws_before,
                    const at::Tensor &ws_after, const at::Tensor &u_after, const at::Tensor &reset_cnt, const at::Tensor &reset_mult,
                    at::Tensor w, at::Tensor q, at::Tensor best_loss, at::Tensor no_improve, at::Tensor n_iter, at::Tensor unfinished) {
    check(abi().fit_sgd_epochs(static_cast<int32_t>(n_users), static_cast<int32_t>(n_items), ptr<const int32_t>(cptr), ptr<const int32_t>(ttime),
                               ptr<const float>(tval), nnz, ptr<const int32_t>(targets), static_cast<int32_t>(targets.numel()),
                               ptr<const int32_t>(sel), ptr<const int32_t>(sel_count), static_cast<int32_t>(cap),
                               static_cast<int32_t>(first_epoch), static_cast<int32_t>(n_epochs), static_cast<int32_t>(max_iter), tol,
                               ptr<const double>(eta), ptr<const double>(ws_before), ptr<const double>(ws_after), ptr<const double>(u_after),
                               ptr<const int32_t>(reset_cnt), ptr<const float>(reset_mult), ptr<float>(w), ptr<float>(q),
                               ptr<double>(best_loss), ptr<int32_t>(no_improve), ptr<int32_t>(n_iter), ptr<int32_t>(unfinished),
                               stream_of(w)), "rtrec_slim_fit_sgd_epochs");
}

void first_touch_aux(const OT &row_ids, const at::Tensor &xb_ptr, const at::Tensor &xb_col, int64_t n_rows, int64_t n_items,
                     const at::Tensor &wc_ptr, const at::Tensor &wc_row, int64_t top_k, const at::Tensor &ids, const at::Tensor &count,
                     at::Tensor aux) {
    check(abi().first_touch_aux(static_cast<int32_t>(n_rows), ptr<const int32_t>(row_ids), ptr<const int32_t>(xb_ptr), ptr<const int32_t>(xb_col),
                                static_cast<int32_t>(xb_ptr.size(0)) - 1, static_cast<int32_t>(n_items), ptr<const int32_t>(wc_ptr),
                                ptr<const int32_t>(wc_row), static_cast<int32_t>(top_k), ptr<const int32_t>(ids), ptr<const int32_t>(count),
                                ptr<uint32_t>(aux), stream_of(aux)), "rtrec_slim_first_touch_aux");
}

void dense_fill(const OT &row_ids, const at::Tensor &xb_ptr, const at::Tensor &xb_col, int64_t n_rows, int64_t col_lo, int64_t col_hi,
                int64_t top_k, bool filter_interacted, at::Tensor ids, at::Tensor scores, at::Tensor aux, at::Tensor count,
                const at::Tensor &flagged_in, at::Tensor flagged_out) {
    check(abi().dense_fill(static_cast<int32_t>(n_rows), ptr<const int32_t>(row_ids), ptr<const int32_t>(xb_ptr), ptr<const int32_t>(xb_col),
                           static_cast<int32_t>(xb_ptr.size(0)) - 1, static_cast<int32_t>(col_lo), static_cast<int32_t>(col_hi),
                           static_cast<int32_t>(top_k), filter_interacted ? 1 : 0, ptr<int32_t>(ids), ptr<float>(scores), ptr<uint32_t>(aux),
                           ptr<int32_t>(count), ptr<const int32_t>(flagged_in), ptr<int32_t>(flagged_out), stream_of(ids)),
          "rtrec_slim_dense_fill");
}

void refine_topk_f64(const OT &row_ids, const at::Tensor &xb_ptr, const at::Tensor &xb_col, const at::Tensor &xb_val, int64_t n_rows,
                     int64_t n_items, const at::Tensor &wc_ptr, const at::Tensor &wc_row, const at::Tensor &wc_val, int64_t top_k,
                     const at::Tensor &in_ids, const at::Tensor &in_scores, const at::Tensor &in_count, double rel_margin,
                     const OT &abs_slack, at::Tensor out_ids, at::Tensor out_scores, at::Tensor out_scores64, at::Tensor out_count,
                     at::Tensor flagged) {
    check(abi().refine_topk_f64(static_cast<int32_t>(n_rows), ptr<const int32_t>(row_ids), ptr<const int32_t>(xb_ptr), ptr<const int32_t>(xb_col),
                                ptr<const float>(xb_val), static_cast<int32_t>(xb_ptr.size(0)) - 1, static_cast<int32_t>(n_items),
                                ptr<const int32_t>(wc_ptr), ptr<const int32_t>(wc_row), ptr<const float>(wc_val), static_cast<int32_t>(top_k),
                                ptr<const int32_t>(in_ids), ptr<const float>(in_scores), ptr<const int32_t>(in_count), rel_margin,
                                ptr<const double>(abs_slack), ptr<int32_t>(out_ids), ptr<float>(out_scores), ptr<double>(out_scores64),
                                ptr<int32_t>(out_count), ptr<int32_t>(flagged), stream_of(out_ids)), "rtrec_slim_refine_topk_f64");
}

void score_candidates(const OT &row_ids, const at::Tensor &xb_ptr, const at::Tensor &xb_col, const at::Tensor &xb_val, int64_t n_rows,
                      int64_t n_items, const at::Tensor &wc_ptr, const at::Tensor &wc_row, const at::Tensor &wc_val, const at::Tensor &cands,
                      int64_t top_k, bool acc_f64, at::Tensor ids, at::Tensor scores, OT scores64, at::Tensor count) {
    check(abi().score_candidates(static_cast<int32_t>(n_rows), ptr<const int32_t>(row_ids), ptr<const int32_t>(xb_ptr), ptr<const int32_t>(xb_col),
                                 ptr<const float>(xb_val), static_cast<int32_t>(xb_ptr.size(0)) - 1, static_cast<int32_t>(n_items),
                                 ptr<const int32_t>(wc_ptr), ptr<const int32_t>(wc_row), ptr<const float>(wc_val), ptr<const int32_t>(cands),
                                 static_cast<int32_t>(cands.numel()), static_cast<int32_t>(top_k), acc_f64 ? 1 : 0, ptr<int32_t>(ids),
                                 ptr<float>(scores), ptr<double>(scores64), ptr<int32_t>(count), stream_of(ids)), "rtrec_slim_score_candidates");
}

// returns {n_cols, n_rows, tile_cols, n_tiles} of the segment layout (the C-ABI writes them to host memory after its own sync)
std::vector<int64_t> seg_plan(const at::Tensor &rows, const at::Tensor &cols, int64_t n_items, int64_t col_lo, int64_t col_hi,
                              const at::Tensor &labels, at::Tensor ws) {
    TORCH_CHECK(cols.numel() == rows.numel(), "seg_plan: rows and cols must have one length");
    int32_t out[4] = {0, 0, 0, 0};
    check(abi().seg_plan(static_cast<int32_t>(n_items), rows.numel(), ptr<const int64_t>(rows), ptr<const int64_t>(cols),
                         static_cast<int32_t>(col_lo), static_cast<int32_t>(col_hi), ptr<const int64_t>(labels), ptr(ws),
                         static_cast<size_t>(ws.numel()), out, stream_of(ws)), "rtrec_slim_seg_plan");
    return {out[0], out[1], out[2], out[3]};
}

void seg_fill(const at::Tensor &rows, const at::Tensor &cols, const at::Tensor &vals, int64_t n_items, int64_t col_lo, int64_t col_hi,
              const at::Tensor &plan_ws, int64_t n_cols, int64_t n_rows, int64_t tile_cols, int64_t n_tiles, at::Tensor ws, at::Tensor info,
              at::Tensor seg_ptr, at::Tensor ent, at::Tensor bound, at::Tensor col_ids, at::Tensor trow_ptr, at::Tensor trow) {
    TORCH_CHECK(cols.numel() == rows.numel() && vals.numel() == rows.numel(), "seg_fill: rows, cols and vals must have one length");
    check(abi().seg_fill(static_cast<int32_t>(n_items), rows.numel(), ptr<const int64_t>(rows), ptr<const int64_t>(cols), ptr<const float>(vals),
                         static_cast<int32_t>(col_lo), static_cast<int32_t>(col_hi), ptr<const void>(plan_ws), static_cast<int32_t>(n_cols),
                         static_cast<int32_t>(n_rows), static_cast<int32_t>(tile_cols), static_cast<int32_t>(n_tiles), ptr(ws),
                         static_cast<size_t>(ws.numel()), ptr<int32_t>(info), ptr<int32_t>(seg_ptr), ptr<int32_t>(ent), ent.size(0),
                         ptr<uint32_t>(bound), ptr<int32_t>(col_ids), ptr<int32_t>(trow_ptr), ptr<int32_t>(trow), trow.size(0),
                         stream_of(info)), "rtrec_slim_seg_fill");
}

void ordered_sums(const at::Tensor &values, const at::Tensor &offsets, int64_t mode, at::Tensor out) {
    TORCH_CHECK(offsets.numel() == out.numel() + 1, "ordered_sums: offsets must hold one more entry than out");
    check(abi().ordered_sums(ptr<const float>(values), ptr<const int64_t>(offsets), static_cast<int32_t>(out.numel()),
                             static_cast<int32_t>(mode), ptr<float>(out), stream_of(out)), "rtrec_slim_ordered_sums");
}

// ---- the checks of the ops from here down
bool has(const OT &t) { return t.has_value() && t->defined(); }

// The pointer a slot of element type T takes.  Every tensor is checked even when it is empty (ptr<> skips those: the ops above hand
// it empty placeholders): an empty call is still a typed call.  nullptr for an empty or absent tensor.
template <typename T>
T *cptr(const at::Tensor &t) {
    check_tensor<T>(t);
    return t.numel() == 0 ? nullptr : static_cast<T *>(t.data_ptr());
}
template <typename T>
T *cptr(const OT &t) { return has(t) ? cptr<T>(*t) : nullptr; }

void one_device(const char *op, const at::Tensor &ref, std::initializer_list<const at::Tensor *> tensors,
                std::initializer_list<const OT *> optionals = {}) {
    for (const at::Tensor *t : tensors) TORCH_CHECK(t->device() == ref.device(), op, ": all tensors must live on one device");
    for (const OT *t : optionals) TORCH_CHECK(!has(*t) || (*t)->device() == ref.device(), op, ": all tensors must live on one device");
}

void check_waves(const char *op, int64_t w) {
    TORCH_CHECK(w == 0 || w == 1 || w == 4, op, ": waves_per_row must be 0, 1 or 4, got ", w);
}

void check_rows_items(const char *op, int64_t rows, int64_t n_items) {
    TORCH_CHECK(rows <= INT32_MAX && n_items >= 0 && n_items < INT32_MAX, op, ": too many rows or items");
}

// One list per row: <name>ids [n_rows, >= k], <name>scores of that form (or null), counts [n_rows] (null: the caller checks them);
// kname is what the messages call k.  rows < 0: ids decides the row count, which is returned.
int64_t check_list(const char *op, const char *name, const char *kname, const at::Tensor &ids, const at::Tensor *scores,
                   const at::Tensor *counts, int64_t k, int64_t rows = -1) {
    TORCH_CHECK(ids.dim() == 2 && (rows < 0 || ids.size(0) == rows) && ids.size(1) >= k, op, ": ", name, "ids must be [n_rows, >= ", kname, "]");
    rows = ids.size(0);
    TORCH_CHECK(!scores || (scores->dim() == 2 && scores->size(0) == rows && scores->size(1) >= k), op, ": ", name,
                "scores must be [n_rows, >= ", kname, "]");
    TORCH_CHECK(!counts || counts->numel() == rows, op, ": ", name, "counts must hold one entry per row");
    return rows;
}

// ids / counts: the lists of score_topk; truth_* the ground truth as CSR over the same rows (include/rtrec_amd.h).  rel is an
// int64 tensor that receives the uint64 relevance words.
void rank_metrics(const at::Tensor &ids, const at::Tensor &counts, const at::Tensor &truth_ptr, const at::Tensor &truth_items,
                  const at::Tensor &truth_len, const at::Tensor &discount, const at::Tensor &ideal, int64_t size, at::Tensor metrics,
                  at::Tensor tp, at::Tensor rel) {
    TORCH_CHECK(size >= 1 && size <= 64, "rank_metrics: size must lie in 1..64, got ", size);
    const int64_t n = check_list("rank_metrics", "", "size", ids, nullptr, nullptr, size);
    TORCH_CHECK(n <= INT32_MAX, "rank_metrics: too many rows");
    TORCH_CHECK(truth_ptr.numel() == n + 1, "rank_metrics: truth_ptr must hold n_rows + 1 entries, got ", truth_ptr.numel());
    TORCH_CHECK(counts.numel() == n && truth_len.numel() == n, "rank_metrics: counts and truth_len must hold one entry per row");
    TORCH_CHECK(discount.numel() == size && ideal.numel() == size + 1, "rank_metrics: discount[size] and ideal[size + 1] expected");
    TORCH_CHECK(metrics.numel() == n * 8 && tp.numel() == n && rel.numel() == n, "rank_metrics: outputs must be metrics[n_rows, 8], tp[n_rows], rel[n_rows]");
    check(abi().rank_metrics(static_cast<int32_t>(n), static_cast<int32_t>(size), cptr<const int32_t>(ids), static_cast<int32_t>(ids.size(1)),
                             cptr<const int32_t>(counts), cptr<const int64_t>(truth_ptr), cptr<const int32_t>(truth_items), truth_items.numel(),
                             cptr<const int32_t>(truth_len), cptr<const double>(discount), cptr<const double>(ideal),
                             reinterpret_cast<uint64_t *>(cptr<int64_t>(rel)), cptr<int32_t>(tp), cptr<double>(metrics), stream_of(metrics)),
          "rtrec_rank_metrics");
}

// One CSC matrix of n_items columns: ptr [n_items + 1], row and val of one length, int32 / float32 (checked even when empty).
void check_csc(const char *op, const char *name, const at::Tensor &colptr, const at::Tensor &crow, const at::Tensor &cval, int64_t n_items) {
    TORCH_CHECK(colptr.numel() == n_items + 1 && cval.numel() == crow.numel(), op, ": ", name, "_ptr must hold n_items + 1 entries, ", name,
                "_row and ", name, "_val one length");
    check_tensor<const int32_t>(colptr); check_tensor<const int32_t>(crow); check_tensor<const float>(cval);
}

// The inputs explain_topk and score_pairs share: one list per row, optional row_ids [n_rows], X as a CSR triple, W as a CSC triple
// of n_items columns, all on ids' device.  Returns n_rows.
int64_t check_lists_x_w(const char *op, const OT &row_ids, const at::Tensor &xb_ptr, const at::Tensor &xb_col, const at::Tensor &xb_val,
                        int64_t n_items, const at::Tensor &wc_ptr, const at::Tensor &wc_row, const at::Tensor &wc_val,
                        const at::Tensor &ids, const at::Tensor &counts, int64_t list_k) {
    const int64_t n = check_list(op, "", "list_k", ids, nullptr, &counts, list_k);
    check_rows_items(op, n, n_items);
    TORCH_CHECK(!has(row_ids) || row_ids->numel() == n, op, ": row_ids must hold one entry per row");
    TORCH_CHECK(xb_ptr.numel() >= 1 && xb_val.numel() == xb_col.numel(), op, ": xb_ptr / xb_col / xb_val are not one CSR matrix");
    check_csc(op, "wc", wc_ptr, wc_row, wc_val, n_items);
    one_device(op, ids, {&xb_ptr, &xb_col, &xb_val, &wc_ptr, &wc_row, &wc_val, &counts}, {&row_ids});
    return n;
}

// ids [n_rows, >= list_k] / counts [n_rows]: lists of item ids (score_topk's, or any the caller brings); the outputs are
// items / contrib [n_rows, list_k, top_m] and support [n_rows, list_k] (include/rtrec_amd.h, "EXPLANATIONS").
void explain_topk(const OT &row_ids, const at::Tensor &xb_ptr, const at::Tensor &xb_col, const at::Tensor &xb_val, int64_t n_items,
                  const at::Tensor &wc_ptr, const at::Tensor &wc_row, const at::Tensor &wc_val, const at::Tensor &ids,
                  const at::Tensor &counts, int64_t list_k, int64_t top_m, at::Tensor items, at::Tensor contrib, at::Tensor support) {
    TORCH_CHECK(list_k >= 1 && list_k <= 64, "explain_topk: list_k must lie in 1..64, got ", list_k);
    TORCH_CHECK(top_m >= 1 && top_m <= 32, "explain_topk: top_m must lie in 1..32, got ", top_m);
    const int64_t n = check_lists_x_w("explain_topk", row_ids, xb_ptr, xb_col, xb_val, n_items, wc_ptr, wc_row, wc_val, ids, counts, list_k);
    TORCH_CHECK(items.numel() == n * list_k * top_m && contrib.numel() == n * list_k * top_m && support.numel() == n * list_k,
                "explain_topk: outputs must be items[n_rows, list_k, top_m], contrib[same], support[n_rows, list_k]");
    check(abi().explain_topk(static_cast<int32_t>(n), cptr<const int32_t>(row_ids), cptr<const int32_t>(xb_ptr), cptr<const int32_t>(xb_col),
                             cptr<const float>(xb_val), static_cast<int32_t>(xb_ptr.numel() - 1), xb_col.numel(), static_cast<int32_t>(n_items),
                             cptr<const int32_t>(wc_ptr), cptr<const int32_t>(wc_row), cptr<const float>(wc_val), wc_row.numel(),
                             cptr<const int32_t>(ids), ids.size(1), static_cast<int32_t>(list_k), cptr<const int32_t>(counts),
                             static_cast<int32_t>(top_m), cptr<int32_t>(items), cptr<float>(contrib), cptr<int32_t>(support), stream_of(items)),
          "rtrec_slim_explain_topk");
}

// items [n_q] query item ids; X and W in CSC form; user_mask: optional bitmap of (n_users + 31) / 32 int32 words; the outputs are
// users / scores [n_q, top_n] and count / eligible [n_q]; ws: rtrec_slim_audience_workspace_bytes (include/rtrec_amd.h,
// "AUDIENCE OF AN ITEM").
void audience_topk(const at::Tensor &items, int64_t n_users, const at::Tensor &xc_ptr, const at::Tensor &xc_row, const at::Tensor &xc_val,
                   const at::Tensor &wc_ptr, const at::Tensor &wc_row, const at::Tensor &wc_val, int64_t top_n, bool filter_interacted,
                   const OT &user_mask, at::Tensor users, at::Tensor scores, at::Tensor count, at::Tensor eligible, at::Tensor ws) {
    TORCH_CHECK(top_n >= 1 && top_n <= 1024, "audience_topk: top_n must lie in 1..1024, got ", top_n);
    const int64_t n = items.numel(), n_items = wc_ptr.numel() - 1;
    TORCH_CHECK(items.dim() == 1 && n <= INT32_MAX, "audience_topk: items must be one list of query item ids");
    TORCH_CHECK(n_users >= 0 && n_users < INT32_MAX && n_items >= 0, "audience_topk: n_users out of range or wc_ptr empty");
    check_csc("audience_topk", "xc", xc_ptr, xc_row, xc_val, n_items);             // (n_items is wc_ptr's: X must have W's columns)
    check_csc("audience_topk", "wc", wc_ptr, wc_row, wc_val, n_items);
    TORCH_CHECK(xc_row.numel() <= INT32_MAX && wc_row.numel() <= INT32_MAX, "audience_topk: xc_row and wc_row must be shorter than 2^31");
    TORCH_CHECK(!has(user_mask) || user_mask->numel() == (n_users + 31) / 32, "audience_topk: user_mask must hold (n_users + 31) / 32 words");
    TORCH_CHECK(users.numel() == n * top_n && scores.numel() == n * top_n && count.numel() == n && eligible.numel() == n,
                "audience_topk: outputs must be users[n_q, top_n], scores[same], count[n_q], eligible[n_q]");
    one_device("audience_topk", items, {&xc_ptr, &xc_row, &xc_val, &wc_ptr, &wc_row, &wc_val, &users, &scores, &count, &eligible, &ws}, {&user_mask});
    check(abi().audience_topk(static_cast<int32_t>(n), cptr<const int32_t>(items), static_cast<int32_t>(n_users), static_cast<int32_t>(n_items),
                              cptr<const int32_t>(xc_ptr), cptr<const int32_t>(xc_row), cptr<const float>(xc_val), xc_row.numel(),
                              cptr<const int32_t>(wc_ptr), cptr<const int32_t>(wc_row), cptr<const float>(wc_val), wc_row.numel(),
                              static_cast<int32_t>(top_n), filter_interacted ? 1 : 0, cptr<const int32_t>(user_mask), cptr<int32_t>(users),
                              cptr<float>(scores), cptr<int32_t>(count), cptr<int32_t>(eligible), cptr<void>(ws),
                              static_cast<size_t>(ws.numel() * ws.element_size()), stream_of(users)),
          "rtrec_slim_audience_topk");
}

// ids [n_rows, >= list_k] / counts [n_rows]: one list of item ids per row; the outputs are scores / support [n_rows, list_k] for
// every position and, with top_k > 0, order [n_rows, top_k] (list positions by rank) / count [n_rows]; with top_k == 0 order and
// count are empty tensors (include/rtrec_amd.h, "RERANK PER-USER CANDIDATE LISTS").
void score_pairs(const OT &row_ids, const at::Tensor &xb_ptr, const at::Tensor &xb_col, const at::Tensor &xb_val, int64_t n_items,
                 const at::Tensor &wc_ptr, const at::Tensor &wc_row, const at::Tensor &wc_val, const at::Tensor &ids,
                 const at::Tensor &counts, int64_t list_k, int64_t top_k, bool filter_interacted, int64_t waves_per_row,
                 at::Tensor scores, at::Tensor support, at::Tensor order, at::Tensor count) {
    TORCH_CHECK(list_k >= 1 && list_k <= 1024, "score_pairs: list_k must lie in 1..1024, got ", list_k);
    TORCH_CHECK(top_k >= 0 && top_k <= list_k, "score_pairs: top_k must lie in 0..list_k, got ", top_k);
    check_waves("score_pairs", waves_per_row);
    const int64_t n = check_lists_x_w("score_pairs", row_ids, xb_ptr, xb_col, xb_val, n_items, wc_ptr, wc_row, wc_val, ids, counts, list_k);
    TORCH_CHECK(scores.numel() == n * list_k && support.numel() == n * list_k, "score_pairs: scores and support must be [n_rows, list_k]");
    TORCH_CHECK(order.numel() == n * top_k && count.numel() == (top_k > 0 ? n : count.numel()) && (count.numel() == n || count.numel() == 0),
                "score_pairs: outputs must be order[n_rows, top_k] and count[n_rows] (count may be empty when top_k == 0)");
    one_device("score_pairs", ids, {&scores, &support, &order, &count});
    check(abi().score_pairs(static_cast<int32_t>(n), cptr<const int32_t>(row_ids), cptr<const int32_t>(xb_ptr), cptr<const int32_t>(xb_col),
                            cptr<const float>(xb_val), static_cast<int32_t>(xb_ptr.numel() - 1), xb_col.numel(), static_cast<int32_t>(n_items),
                            cptr<const int32_t>(wc_ptr), cptr<const int32_t>(wc_row), cptr<const float>(wc_val), wc_row.numel(),
                            cptr<const int32_t>(ids), ids.size(1), static_cast<int32_t>(list_k), cptr<const int32_t>(counts),
                            static_cast<int32_t>(top_k), filter_interacted ? 1 : 0, static_cast<int32_t>(waves_per_row), cptr<float>(scores),
                            cptr<int32_t>(support), cptr<int32_t>(order), cptr<int32_t>(count), stream_of(scores)),
          "rtrec_slim_score_pairs");
}

// ids / scores [n_rows, >= list_k] / counts [n_rows]: one list of item ids and base scores per row; W as a CSC triple of n_items
// columns; the outputs are order / value / penalty [n_rows, keep] and count [n_rows] (include/rtrec_amd_ext.h, "DIVERSIFIED LISTS").
void diversify_lists(const at::Tensor &wc_ptr, const at::Tensor &wc_row, const at::Tensor &wc_val, int64_t n_items, const at::Tensor &ids,
                     const at::Tensor &scores, const at::Tensor &counts, int64_t list_k, int64_t keep, double lam, int64_t waves_per_row,
                     at::Tensor order, at::Tensor value, at::Tensor penalty, at::Tensor count) {
    TORCH_CHECK(list_k >= 1 && list_k <= 1024, "diversify_lists: list_k must lie in 1..1024, got ", list_k);
    TORCH_CHECK(keep >= 1 && keep <= list_k, "diversify_lists: keep must lie in 1..list_k, got ", keep);
    TORCH_CHECK(lam >= 0.0 && lam <= 1.0, "diversify_lists: lam must lie in [0, 1], got ", lam);
    check_waves("diversify_lists", waves_per_row);
    const int64_t n = check_list("diversify_lists", "", "list_k", ids, &scores, &counts, list_k);
    check_rows_items("diversify_lists", n, n_items);
    TORCH_CHECK(order.numel() == n * keep && value.numel() == n * keep && penalty.numel() == n * keep && count.numel() == n,
                "diversify_lists: outputs must be order[n_rows, keep], value[same], penalty[same], count[n_rows]");
    check_csc("diversify_lists", "wc", wc_ptr, wc_row, wc_val, n_items);
    one_device("diversify_lists", ids, {&wc_ptr, &wc_row, &wc_val, &scores, &counts, &order, &value, &penalty, &count});
    check(abi().diversify_lists(static_cast<int32_t>(n), static_cast<int32_t>(n_items), cptr<const int32_t>(wc_ptr), cptr<const int32_t>(wc_row),
                                cptr<const float>(wc_val), wc_row.numel(), cptr<const int32_t>(ids), ids.size(1), cptr<const float>(scores),
                                scores.size(1), static_cast<int32_t>(list_k), cptr<const int32_t>(counts), static_cast<int32_t>(keep),
                                static_cast<float>(lam), static_cast<int32_t>(waves_per_row), cptr<int32_t>(order), cptr<float>(value),
                                cptr<float>(penalty), cptr<int32_t>(count), stream_of(order)),
          "rtrec_slim_diversify_lists");
}

// ids [n_rows, >= list_k] / counts [n_rows]: one list of item ids per row; W as a CSC triple of n_items columns; item_weight
// (float32) and exposure (int32, ADDED to, never zeroed) hold n_items entries each and may be absent; the outputs are n / sim_sum /
// linked / weight_sum [n_rows] (include/rtrec_amd_ext.h, "LIST QUALITY").
void list_quality(const at::Tensor &wc_ptr, const at::Tensor &wc_row, const at::Tensor &wc_val, int64_t n_items, const at::Tensor &ids,
                  const at::Tensor &counts, int64_t list_k, const OT &item_weight, int64_t waves_per_row, at::Tensor n, at::Tensor sim_sum,
                  at::Tensor linked, at::Tensor weight_sum, const OT &exposure) {
    TORCH_CHECK(list_k >= 1 && list_k <= 1024, "list_quality: list_k must lie in 1..1024, got ", list_k);
    check_waves("list_quality", waves_per_row);
    const int64_t rows = check_list("list_quality", "", "list_k", ids, nullptr, &counts, list_k);
    check_rows_items("list_quality", rows, n_items);
    TORCH_CHECK(n.numel() == rows && sim_sum.numel() == rows && linked.numel() == rows && weight_sum.numel() == rows,
                "list_quality: outputs must be n[n_rows], sim_sum[n_rows], linked[n_rows], weight_sum[n_rows]");
    TORCH_CHECK(!has(item_weight) || item_weight->numel() == n_items, "list_quality: item_weight must hold n_items entries");
    TORCH_CHECK(!has(exposure) || exposure->numel() == n_items, "list_quality: exposure must hold n_items entries");
    check_csc("list_quality", "wc", wc_ptr, wc_row, wc_val, n_items);
    one_device("list_quality", ids, {&wc_ptr, &wc_row, &wc_val, &counts, &n, &sim_sum, &linked, &weight_sum}, {&item_weight, &exposure});
    check(abi().list_quality(static_cast<int32_t>(rows), static_cast<int32_t>(n_items), cptr<const int32_t>(wc_ptr), cptr<const int32_t>(wc_row),
                             cptr<const float>(wc_val), wc_row.numel(), cptr<const int32_t>(ids), ids.size(1), static_cast<int32_t>(list_k),
                             cptr<const int32_t>(counts), cptr<const float>(item_weight), cptr<int32_t>(exposure),
                             static_cast<int32_t>(waves_per_row), cptr<int32_t>(n), cptr<float>(sim_sum), cptr<int32_t>(linked),
                             cptr<float>(weight_sum), stream_of(n)),
          "rtrec_slim_list_quality");
}

// scores [n_rows, >= n_items] float32 or float64 (the dtype selects the kernel); the rows of X used for filtering as a CSR without
// values (row_ids: the row of X per score row, absent = row r); the targets as a CSR over the score rows: tg_ptr [n_rows + 1] int64
// into tg_items int32; the outputs are above / tied [n_tg] int32, score [n_tg] float64, competing [n_rows] int32
// (include/rtrec_amd_ext.h, "CATALOGUE RANKS").
void catalogue_ranks(const at::Tensor &scores, int64_t n_items, const OT &row_ids, const at::Tensor &xb_ptr, const at::Tensor &xb_col,
                     bool filter_interacted, int64_t mode, const at::Tensor &tg_ptr, const at::Tensor &tg_items, at::Tensor above,
                     at::Tensor tied, at::Tensor score, at::Tensor competing) {
    TORCH_CHECK(mode == RTREC_TOPK_SPARSE || mode == RTREC_TOPK_DENSE, "catalogue_ranks: mode must be 0 (SPARSE) or 1 (DENSE), got ", mode);
    TORCH_CHECK(scores.dim() == 2, "catalogue_ranks: scores must be [n_rows, >= n_items]");
    const int64_t rows = scores.size(0), n_tg = tg_items.numel();
    check_rows_items("catalogue_ranks", rows, n_items);
    TORCH_CHECK(scores.size(1) >= n_items, "catalogue_ranks: scores must be [n_rows, >= n_items]");
    TORCH_CHECK(scores.scalar_type() == at::kFloat || scores.scalar_type() == at::kDouble, "catalogue_ranks: scores must be float32 or float64, got ",
                scores.scalar_type());
    TORCH_CHECK(tg_ptr.numel() == rows + 1, "catalogue_ranks: tg_ptr must hold n_rows + 1 offsets");
    TORCH_CHECK(above.numel() == n_tg && tied.numel() == n_tg && score.numel() == n_tg && competing.numel() == rows,
                "catalogue_ranks: outputs must be above[n_tg], tied[n_tg], score[n_tg], competing[n_rows]");
    TORCH_CHECK(xb_ptr.numel() >= 1 && xb_ptr.numel() - 1 <= INT32_MAX, "catalogue_ranks: xb_ptr must hold n_x_rows + 1 offsets");
    TORCH_CHECK(!has(row_ids) || row_ids->numel() == rows, "catalogue_ranks: row_ids must hold one entry per row");
    one_device("catalogue_ranks", scores, {&xb_ptr, &xb_col, &tg_ptr, &tg_items, &above, &tied, &score, &competing}, {&row_ids});
    const bool f64 = scores.scalar_type() == at::kDouble;
    const void *d_scores = f64 ? static_cast<const void *>(cptr<const double>(scores)) : cptr<const float>(scores);
    check(abi().catalogue_ranks(static_cast<int32_t>(rows), static_cast<int32_t>(n_items), d_scores, scores.size(1), f64 ? 1 : 0,
                                cptr<const int32_t>(row_ids), cptr<const int32_t>(xb_ptr), cptr<const int32_t>(xb_col),
                                static_cast<int32_t>(xb_ptr.numel() - 1), xb_col.numel(), filter_interacted ? 1 : 0, static_cast<int32_t>(mode),
                                cptr<const int64_t>(tg_ptr), cptr<const int32_t>(tg_items), n_tg, cptr<int32_t>(above), cptr<int32_t>(tied),
                                cptr<double>(score), cptr<int32_t>(competing), stream_of(competing)),
          "rtrec_slim_catalogue_ranks");
}

// a_ids / a_scores [n_rows, >= ka] / a_counts [n_rows] and the same for b: two lists of item ids and scores per row; with
// `contacts` the rows of X as a CSR without values (row_ids: the row of X per list row, absent = row r) and, optionally, the count
// CSR cn_* (int32) over the same rows; the outputs are ids / value / source [n_rows, keep] and count [n_rows]
// (include/rtrec_amd_ext.h, "BLENDED LISTS").
void blend_lists(int64_t n_items, const at::Tensor &a_ids, const at::Tensor &a_scores, const at::Tensor &a_counts, int64_t ka,
                 const at::Tensor &b_ids, const at::Tensor &b_scores, const at::Tensor &b_counts, int64_t kb, int64_t keep, double weight_b,
                 bool contacts, double k, bool mnz, const OT &row_ids, const OT &xb_ptr, const OT &xb_col, const OT &cn_ptr, const OT &cn_col,
                 const OT &cn_val, int64_t waves_per_row, at::Tensor ids, at::Tensor value, at::Tensor source, at::Tensor count) {
    TORCH_CHECK(ka >= 1 && ka <= 1024 && kb >= 1 && kb <= 1024, "blend_lists: ka and kb must lie in 1..1024, got ", ka, " and ", kb);
    TORCH_CHECK(keep >= 1 && keep <= ka + kb, "blend_lists: keep must lie in 1..ka+kb, got ", keep);
    TORCH_CHECK(weight_b >= 0.0 && k >= 0.0, "blend_lists: weight_b and k must lie in [0, inf], got ", weight_b, " and ", k);
    check_waves("blend_lists", waves_per_row);
    const int64_t rows = check_list("blend_lists", "a_", "ka", a_ids, &a_scores, nullptr, ka);
    check_list("blend_lists", "b_", "kb", b_ids, &b_scores, nullptr, kb, rows);
    check_rows_items("blend_lists", rows, n_items);
    TORCH_CHECK(a_counts.numel() == rows && b_counts.numel() == rows, "blend_lists: a_counts and b_counts must hold one entry per row");
    TORCH_CHECK(ids.numel() == rows * keep && value.numel() == rows * keep && source.numel() == rows * keep && count.numel() == rows,
                "blend_lists: outputs must be ids[n_rows, keep], value[same], source[same], count[n_rows]");
    int64_t n_x_rows = 0, xb_nnz = 0, cn_nnz = 0;
    if (contacts) {
        TORCH_CHECK(has(xb_ptr) && has(xb_col), "blend_lists: contacts need xb_ptr and xb_col");
        TORCH_CHECK(xb_ptr->numel() >= 1 && xb_ptr->numel() - 1 <= INT32_MAX, "blend_lists: xb_ptr must hold n_x_rows + 1 offsets");
        n_x_rows = xb_ptr->numel() - 1;
        xb_nnz = xb_col->numel();
        TORCH_CHECK(!has(row_ids) || row_ids->numel() == rows, "blend_lists: row_ids must hold one entry per row");
        if (has(cn_ptr)) {
            TORCH_CHECK(has(cn_col) && has(cn_val), "blend_lists: cn_ptr comes with cn_col and cn_val");
            TORCH_CHECK(cn_ptr->numel() == n_x_rows + 1, "blend_lists: cn_ptr must hold n_x_rows + 1 offsets");
            TORCH_CHECK(cn_col->numel() == cn_val->numel(), "blend_lists: cn_col and cn_val must have one length");
            cn_nnz = cn_col->numel();
        }
        one_device("blend_lists", a_ids, {}, {&row_ids, &xb_ptr, &xb_col, &cn_ptr, &cn_col, &cn_val});
    }
    one_device("blend_lists", a_ids, {&a_scores, &a_counts, &b_ids, &b_scores, &b_counts, &ids, &value, &source, &count});
    const bool counted = contacts && has(cn_ptr);
    check(abi().blend_lists(static_cast<int32_t>(rows), static_cast<int32_t>(n_items), cptr<const int32_t>(a_ids), a_ids.size(1),
                            cptr<const float>(a_scores), a_scores.size(1), cptr<const int32_t>(a_counts), static_cast<int32_t>(ka),
                            cptr<const int32_t>(b_ids), b_ids.size(1), cptr<const float>(b_scores), b_scores.size(1), cptr<const int32_t>(b_counts),
                            static_cast<int32_t>(kb), static_cast<int32_t>(keep), static_cast<float>(weight_b),
                            contacts ? RTREC_BLEND_CONTACTS : RTREC_BLEND_CONSTANT, k, mnz ? 1 : 0,
                            contacts ? cptr<const int32_t>(row_ids) : nullptr, contacts ? cptr<const int32_t>(xb_ptr) : nullptr,
                            contacts ? cptr<const int32_t>(xb_col) : nullptr, static_cast<int32_t>(n_x_rows), xb_nnz,
                            counted ? cptr<const int32_t>(cn_ptr) : nullptr, counted ? cptr<const int32_t>(cn_col) : nullptr,
                            counted ? cptr<const int32_t>(cn_val) : nullptr, cn_nnz, static_cast<int32_t>(waves_per_row), cptr<int32_t>(ids),
                            cptr<float>(value), cptr<int32_t>(source), cptr<int32_t>(count), stream_of(count)),
          "rtrec_slim_blend_lists");
}

// What factor_topk and factor_similar_topk share (the scan of csrc/factor_scan.hip.h): the ranges of dim, top_k and item_splits,
// qt [>= dim, >= n_items], ids / scores [n_rows, top_k], item_mask [>= n_items] uint8 / bool.  Returns the workspace's bytes.
size_t check_factor_scan(const char *op, int64_t dim, int64_t top_k, int64_t item_splits, int64_t rows, int64_t n_items, const at::Tensor &qt,
                         const at::Tensor &ids, const at::Tensor &scores, const OT &item_mask, const OT &workspace) {
    TORCH_CHECK(dim >= 1 && dim <= 256, op, ": dim must lie in 1..256, got ", dim);
    TORCH_CHECK(top_k >= 1 && top_k <= 128, op, ": top_k must lie in 1..128, got ", top_k);
    TORCH_CHECK(item_splits >= 0 && item_splits <= 64, op, ": item_splits must lie in 0..64, got ", item_splits);
    TORCH_CHECK(qt.dim() == 2 && qt.size(0) >= dim && qt.size(1) >= n_items, op, ": qt must be [>= dim, >= n_items]");
    TORCH_CHECK(ids.numel() == rows * top_k && scores.numel() == rows * top_k, op, ": outputs must be ids[n_rows, top_k], scores[same], count[n_rows]");
    TORCH_CHECK(!has(item_mask) || (item_mask->numel() >= n_items && (item_mask->scalar_type() == at::kByte || item_mask->scalar_type() == at::kBool)),
                op, ": item_mask must hold one uint8 / bool entry per item");
    return has(workspace) ? static_cast<size_t>(workspace->numel()) * workspace->element_size() : 0;
}

// p [n_p_rows, >= dim] float32: one vector per row; qt [>= dim, >= n_items] float32: the item vectors component-major; one job
// per entry of count: row_ids names its row of X (absent = row r), p_index [n_x_rows] the vector of a row of X (absent = row x);
// item_mask [>= n_items] uint8 / bool; xb_* the rows of X as a CSR without values (only with filter_interacted); the outputs are
// ids / scores [n_rows, top_k] and count [n_rows]; workspace: bytes for the partial lists of item_splits chunks
// (include/rtrec_amd_ext.h, "FACTOR TOP-K").
void factor_topk(const OT &row_ids, const OT &p_index, int64_t n_x_rows, const at::Tensor &p, const at::Tensor &qt, int64_t n_items,
                 int64_t dim, const OT &item_mask, const OT &xb_ptr, const OT &xb_col, bool filter_interacted, int64_t top_k,
                 int64_t item_splits, at::Tensor ids, at::Tensor scores, at::Tensor count, const OT &workspace) {
    const int64_t rows = count.numel();
    const size_t ws_bytes = check_factor_scan("factor_topk", dim, top_k, item_splits, rows, n_items, qt, ids, scores, item_mask, workspace);
    TORCH_CHECK(rows <= INT32_MAX && n_items >= 0 && n_items < INT32_MAX && n_x_rows >= 0 && n_x_rows < INT32_MAX,
                "factor_topk: too many rows or items");
    TORCH_CHECK(p.dim() == 2 && p.size(1) >= dim && p.size(0) <= INT32_MAX, "factor_topk: p must be [n_p_rows, >= dim]");
    TORCH_CHECK(!has(row_ids) || row_ids->numel() == rows, "factor_topk: row_ids must hold one entry per job");
    TORCH_CHECK(!has(p_index) || p_index->numel() == n_x_rows, "factor_topk: p_index must hold one entry per row of X");
    int64_t xb_nnz = 0;
    if (filter_interacted) {
        TORCH_CHECK(has(xb_ptr) && has(xb_col), "factor_topk: filter_interacted needs xb_ptr and xb_col");
        TORCH_CHECK(xb_ptr->numel() == n_x_rows + 1, "factor_topk: xb_ptr must hold n_x_rows + 1 offsets");
        xb_nnz = xb_col->numel();
    }
    one_device("factor_topk", count, {&p, &qt, &ids, &scores}, {&row_ids, &p_index, &item_mask, &xb_ptr, &xb_col, &workspace});
    check(abi().factor_topk(static_cast<int32_t>(rows), cptr<const int32_t>(row_ids), cptr<const int32_t>(p_index),
                            static_cast<int32_t>(n_x_rows), cptr<const float>(p), p.size(1), static_cast<int32_t>(p.size(0)),
                            cptr<const float>(qt), qt.size(1), static_cast<int32_t>(n_items), static_cast<int32_t>(dim),
                            static_cast<const uint8_t *>(cptr<const void>(item_mask)),
                            filter_interacted ? cptr<const int32_t>(xb_ptr) : nullptr, filter_interacted ? cptr<const int32_t>(xb_col) : nullptr,
                            xb_nnz, filter_interacted ? 1 : 0, static_cast<int32_t>(top_k), static_cast<int32_t>(item_splits),
                            cptr<int32_t>(ids), cptr<float>(scores), cptr<int32_t>(count), cptr<void>(workspace), ws_bytes, stream_of(count)),
          "rtrec_factor_topk");
}

// f_ptr [n_f_rows + 1] / f_col [nnz] / f_val [nnz] (absent = all ones): the feature rows as a CSR; e [n_features, >= dim_e] float32
// and bias [n_features] (needed by layout 1 / 2): the per-feature table; job_rows [n_jobs] names the row of a job (absent = row r);
// slot c of job r is written to out.flatten()[r * row_stride + c * comp_stride] (out: any contiguous float32 tensor that holds the
// last slot), has [n_jobs] uint8 (include/rtrec_amd_ext.h, "FEATURE REPRESENTATIONS").
void feature_repr(const OT &job_rows, const at::Tensor &f_ptr, const at::Tensor &f_col, const OT &f_val, const at::Tensor &e, int64_t dim_e,
                  const OT &bias, int64_t layout, int64_t n_jobs, at::Tensor out, int64_t row_stride, int64_t comp_stride, const OT &has_out) {
    TORCH_CHECK(layout >= 0 && layout <= 2, "feature_repr: layout must be 0 (plain), 1 (user stacking) or 2 (item stacking), got ", layout);
    const int64_t width = dim_e + (layout == 0 ? 0 : 2);
    TORCH_CHECK(dim_e >= 1 && width <= 256, "feature_repr: dim_e must lie in 1..", 256 - (layout == 0 ? 0 : 2), ", got ", dim_e);
    TORCH_CHECK(n_jobs >= 0 && n_jobs <= INT32_MAX, "feature_repr: n_jobs must lie in 0..2^31-1");
    TORCH_CHECK(f_ptr.numel() >= 1 && f_ptr.numel() - 1 <= INT32_MAX, "feature_repr: f_ptr must hold n_f_rows + 1 offsets");
    TORCH_CHECK(e.dim() == 2 && e.size(1) >= dim_e && e.size(0) <= INT32_MAX, "feature_repr: e must be [n_features, >= dim_e]");
    TORCH_CHECK(!has(f_val) || f_val->numel() == f_col.numel(), "feature_repr: f_val must hold one value per entry of f_col");
    TORCH_CHECK(!has(job_rows) || job_rows->numel() == n_jobs, "feature_repr: job_rows must hold one entry per job");
    TORCH_CHECK(layout == 0 || (has(bias) && bias->numel() == e.size(0)), "feature_repr: a stacking layout needs one bias per feature");
    TORCH_CHECK((comp_stride == 1 && row_stride >= width) || (row_stride == 1 && comp_stride >= n_jobs),
                "feature_repr: the output is row-major (comp_stride 1, row_stride >= width) or component-major (row_stride 1, "
                "comp_stride >= n_jobs), got row_stride ", row_stride, " and comp_stride ", comp_stride);
    TORCH_CHECK(n_jobs == 0 || out.numel() > (n_jobs - 1) * row_stride + (width - 1) * comp_stride,
                "feature_repr: out does not hold the last slot");
    TORCH_CHECK(!has(has_out) || (has_out->numel() >= n_jobs && (has_out->scalar_type() == at::kByte || has_out->scalar_type() == at::kBool)),
                "feature_repr: has must hold one uint8 / bool entry per job");
    one_device("feature_repr", out, {&f_ptr, &f_col, &e}, {&job_rows, &f_val, &bias, &has_out});
    check(abi().feature_repr(static_cast<int32_t>(n_jobs), cptr<const int32_t>(job_rows), static_cast<int32_t>(f_ptr.numel() - 1),
                             cptr<const int32_t>(f_ptr), cptr<const int32_t>(f_col), cptr<const float>(f_val), f_col.numel(),
                             cptr<const float>(e), e.size(1), static_cast<int32_t>(e.size(0)), static_cast<int32_t>(dim_e),
                             cptr<const float>(bias), static_cast<int32_t>(layout), cptr<float>(out), row_stride, comp_stride,
                             static_cast<uint8_t *>(cptr<void>(has_out)), stream_of(out)),
          "rtrec_feature_repr");
}

// v: any contiguous float32 tensor; component c of vector r is v.flatten()[r * row_stride + c * comp_stride]; out [n] float32
// (include/rtrec_amd_ext.h, "FACTOR NORMS").
void factor_norms(const at::Tensor &v, int64_t n, int64_t dim, int64_t row_stride, int64_t comp_stride, at::Tensor out) {
    TORCH_CHECK(dim >= 1 && dim <= 256, "factor_norms: dim must lie in 1..256, got ", dim);
    TORCH_CHECK(n >= 0 && n <= INT32_MAX, "factor_norms: n must lie in 0..2^31-1");
    TORCH_CHECK((comp_stride == 1 && row_stride >= dim) || (row_stride == 1 && comp_stride >= n),
                "factor_norms: the vectors are row-major (comp_stride 1, row_stride >= dim) or component-major (row_stride 1, "
                "comp_stride >= n), got row_stride ", row_stride, " and comp_stride ", comp_stride);
    TORCH_CHECK(n == 0 || v.numel() > (n - 1) * row_stride + (dim - 1) * comp_stride, "factor_norms: v does not hold the last component");
    TORCH_CHECK(out.numel() == n, "factor_norms: out must hold one entry per vector");
    one_device("factor_norms", out, {&v});
    check(abi().factor_norms(static_cast<int32_t>(n), cptr<const float>(v), row_stride, comp_stride, static_cast<int32_t>(dim),
                             cptr<float>(out), stream_of(out)),
          "rtrec_factor_norms");
}

// queries [n_rows] int32 (absent only with p); p [n_rows, >= dim] / p_norms [n_rows]: brought query vectors (absent: the vectors
// are columns of qt); qt [>= dim, >= n_items] float32 component-major; norms [>= n_items]; item_mask [>= n_items] uint8 / bool;
// the outputs are ids / scores [n_rows, top_k], count [n_rows] and, optionally, div [n_rows]; workspace as for factor_topk
// (include/rtrec_amd_ext.h, "FACTOR SIMILAR TOP-K").
void factor_similar_topk(const OT &queries, const OT &p, const OT &p_norms, const at::Tensor &qt, int64_t n_items, int64_t dim,
                         const at::Tensor &norms, const OT &item_mask, int64_t top_k, int64_t item_splits, bool write_cosine,
                         at::Tensor ids, at::Tensor scores, at::Tensor count, const OT &div, const OT &workspace) {
    const int64_t rows = count.numel();
    const size_t ws_bytes = check_factor_scan("factor_similar_topk", dim, top_k, item_splits, rows, n_items, qt, ids, scores, item_mask, workspace);
    check_rows_items("factor_similar_topk", rows, n_items);
    TORCH_CHECK(norms.numel() >= n_items, "factor_similar_topk: norms must hold one entry per item");
    TORCH_CHECK(!has(div) || div->numel() == rows, "factor_similar_topk: div must hold one entry per job");
    if (has(p)) {
        TORCH_CHECK(p->dim() == 2 && p->size(0) == rows && p->size(1) >= dim, "factor_similar_topk: p must be [n_rows, >= dim]");
        TORCH_CHECK(has(p_norms) && p_norms->numel() == rows, "factor_similar_topk: p comes with p_norms, one entry per job");
        TORCH_CHECK(!has(queries) || queries->numel() == rows, "factor_similar_topk: queries must hold one entry per job");
    } else {
        TORCH_CHECK(has(queries) && queries->numel() == rows, "factor_similar_topk: queries must hold one entry per job");
    }
    one_device("factor_similar_topk", count, {&qt, &norms, &ids, &scores}, {&queries, &p, &p_norms, &item_mask, &div, &workspace});
    const bool brought = has(p) && rows > 0;
    check(abi().factor_similar_topk(static_cast<int32_t>(rows), cptr<const int32_t>(queries), brought ? cptr<const float>(p) : nullptr,
                                    brought ? p->size(1) : 0, brought ? cptr<const float>(p_norms) : nullptr, cptr<const float>(qt),
                                    qt.size(1), static_cast<int32_t>(n_items), static_cast<int32_t>(dim), cptr<const float>(norms),
                                    static_cast<const uint8_t *>(cptr<const void>(item_mask)), static_cast<int32_t>(top_k),
                                    static_cast<int32_t>(item_splits), write_cosine ? 1 : 0, cptr<int32_t>(ids), cptr<float>(scores),
                                    cptr<int32_t>(count), cptr<float>(div), cptr<void>(workspace), ws_bytes, stream_of(count)),
          "rtrec_factor_similar_topk");
}

// a_ids / a_scores [n_rows, >= ka] / a_counts [n_rows] and the same for b; a_div [n_rows] float32 and exclude [n_rows] int32 are
// optional; the outputs are ids / source [n_rows, keep] int32, value [n_rows, keep] FLOAT64 and count [n_rows]
// (include/rtrec_amd_ext.h, "SIMILAR BLEND").
void similar_blend(int64_t n_items, const at::Tensor &a_ids, const at::Tensor &a_scores, const at::Tensor &a_counts, int64_t ka,
                   const OT &a_div, const at::Tensor &b_ids, const at::Tensor &b_scores, const at::Tensor &b_counts, int64_t kb,
                   const OT &exclude, int64_t keep, int64_t waves_per_row, at::Tensor ids, at::Tensor value, at::Tensor source,
                   at::Tensor count) {
    TORCH_CHECK(ka >= 1 && ka <= 1024 && kb >= 1 && kb <= 1024, "similar_blend: ka and kb must lie in 1..1024, got ", ka, " and ", kb);
    TORCH_CHECK(keep >= 1 && keep <= ka + kb, "similar_blend: keep must lie in 1..ka+kb, got ", keep);
    check_waves("similar_blend", waves_per_row);
    const int64_t rows = check_list("similar_blend", "a_", "ka", a_ids, &a_scores, nullptr, ka);
    check_list("similar_blend", "b_", "kb", b_ids, &b_scores, nullptr, kb, rows);
    check_rows_items("similar_blend", rows, n_items);
    TORCH_CHECK(a_counts.numel() == rows && b_counts.numel() == rows, "similar_blend: a_counts and b_counts must hold one entry per row");
    TORCH_CHECK((!has(a_div) || a_div->numel() == rows) && (!has(exclude) || exclude->numel() == rows),
                "similar_blend: a_div and exclude must hold one entry per row");
    TORCH_CHECK(ids.numel() == rows * keep && value.numel() == rows * keep && source.numel() == rows * keep && count.numel() == rows,
                "similar_blend: outputs must be ids[n_rows, keep], value[same], source[same], count[n_rows]");
    one_device("similar_blend", a_ids, {&a_scores, &a_counts, &b_ids, &b_scores, &b_counts, &ids, &value, &source, &count}, {&a_div, &exclude});
    check(abi().similar_blend(static_cast<int32_t>(rows), static_cast<int32_t>(n_items), cptr<const int32_t>(a_ids), a_ids.size(1),
                              cptr<const float>(a_scores), a_scores.size(1), cptr<const int32_t>(a_counts), static_cast<int32_t>(ka),
                              cptr<const float>(a_div), cptr<const int32_t>(b_ids), b_ids.size(1), cptr<const float>(b_scores),
                              b_scores.size(1), cptr<const int32_t>(b_counts), static_cast<int32_t>(kb), cptr<const int32_t>(exclude),
                              static_cast<int32_t>(keep), static_cast<int32_t>(waves_per_row), cptr<int32_t>(ids), cptr<double>(value),
                              cptr<int32_t>(source), cptr<int32_t>(count), stream_of(count)),
          "rtrec_similar_blend");
}

// v [>= n_v, v_stride >= dim] float32 row-major: the fixed side of a half-step; gram [dim, dim]; workspace: the partials,
// RTREC_FACTOR_GRAM_WORKSPACE_BYTES(n_v, dim) bytes, absent only with n_v == 0 (include/rtrec_amd_ext.h, "FACTOR GRAM").
void factor_gram(const at::Tensor &v, int64_t n_v, int64_t dim, double reg, at::Tensor gram, const OT &workspace) {
    TORCH_CHECK(dim >= 1 && dim <= 64, "factor_gram: dim must lie in 1..64, got ", dim);
    TORCH_CHECK(n_v >= 0 && n_v <= INT32_MAX, "factor_gram: n_v must lie in 0..2^31-1");
    TORCH_CHECK(v.dim() == 2 && v.size(0) >= n_v && v.size(1) >= dim, "factor_gram: v must be [>= n_v, >= dim]");
    TORCH_CHECK(reg >= 0.0, "factor_gram: reg must be a number >= 0, got ", reg);
    TORCH_CHECK(gram.numel() == dim * dim, "factor_gram: gram must be [dim, dim]");
    const size_t need = RTREC_FACTOR_GRAM_WORKSPACE_BYTES(n_v, dim);
    const size_t ws_bytes = has(workspace) ? static_cast<size_t>(workspace->numel()) * workspace->element_size() : 0;
    TORCH_CHECK(ws_bytes >= need, "factor_gram: the workspace holds ", ws_bytes, " bytes, RTREC_FACTOR_GRAM_WORKSPACE_BYTES(n_v, dim) = ", need);
    one_device("factor_gram", gram, {&v}, {&workspace});
    check(abi().factor_gram(static_cast<int32_t>(n_v), cptr<const float>(v), v.size(1), static_cast<int32_t>(dim), static_cast<float>(reg),
                            cptr<float>(gram), cptr<void>(workspace), ws_bytes, stream_of(gram)),
          "rtrec_factor_gram");
}

// r_ptr [n_rows + 1] / r_idx [nnz] / r_val [nnz]: R as a CSR (int32 / int32 / float32); v [>= n_v, v_stride >= dim] the fixed side
// and gram [dim, dim] its rtrec_factor_gram; job_rows [n_jobs] names the row of a job (absent = row r); out [>= n_rows, out_stride >=
// dim] float32 is written in place, status [n_jobs] uint8 (include/rtrec_amd_ext.h, "FACTOR ALS SOLVE").
void factor_als_solve(const OT &job_rows, int64_t n_jobs, const at::Tensor &r_ptr, const at::Tensor &r_idx, const at::Tensor &r_val,
                      const at::Tensor &v, int64_t n_v, int64_t dim, const at::Tensor &gram, double alpha, at::Tensor out,
                      at::Tensor status) {
    TORCH_CHECK(dim >= 1 && dim <= 64, "factor_als_solve: dim must lie in 1..64, got ", dim);
    TORCH_CHECK(n_jobs >= 0 && n_jobs <= INT32_MAX && n_v >= 0 && n_v <= INT32_MAX, "factor_als_solve: n_jobs and n_v must lie in 0..2^31-1");
    TORCH_CHECK(r_ptr.numel() >= 1 && r_ptr.numel() - 1 <= INT32_MAX, "factor_als_solve: r_ptr must hold n_rows + 1 offsets");
    const int64_t n_rows = r_ptr.numel() - 1;
    TORCH_CHECK(r_val.numel() == r_idx.numel(), "factor_als_solve: r_val must hold one value per entry of r_idx");
    TORCH_CHECK(v.dim() == 2 && v.size(0) >= n_v && v.size(1) >= dim, "factor_als_solve: v must be [>= n_v, >= dim]");
    TORCH_CHECK(gram.numel() == dim * dim, "factor_als_solve: gram must be [dim, dim]");
    TORCH_CHECK(alpha > 0.0, "factor_als_solve: alpha must be a number > 0, got ", alpha);
    TORCH_CHECK(out.dim() == 2 && out.size(0) >= n_rows && out.size(1) >= dim, "factor_als_solve: out must be [>= n_rows, >= dim]");
    TORCH_CHECK(!has(job_rows) || job_rows->numel() == n_jobs, "factor_als_solve: job_rows must hold one entry per job");
    TORCH_CHECK(has(job_rows) || n_jobs <= n_rows, "factor_als_solve: without job_rows there is at most one job per row");
    TORCH_CHECK(status.numel() >= n_jobs && (status.scalar_type() == at::kByte || status.scalar_type() == at::kBool),
                "factor_als_solve: status must hold one uint8 / bool entry per job");
    one_device("factor_als_solve", out, {&r_ptr, &r_idx, &r_val, &v, &gram, &status}, {&job_rows});
    check(abi().factor_als_solve(static_cast<int32_t>(n_jobs), cptr<const int32_t>(job_rows), static_cast<int32_t>(n_rows),
                                 cptr<const int32_t>(r_ptr), cptr<const int32_t>(r_idx), cptr<const float>(r_val), r_idx.numel(),
                                 cptr<const float>(v), v.size(1), static_cast<int32_t>(n_v), static_cast<int32_t>(dim),
                                 cptr<const float>(gram), static_cast<float>(alpha), cptr<float>(out), out.size(1),
                                 static_cast<uint8_t *>(cptr<void>(status)), stream_of(out)),
          "rtrec_factor_als_solve");
}

// factor_gram's arguments for dim in 1..256 (include/rtrec_amd_ext.h, "FACTOR GRAM WIDE").
void factor_gram_wide(const at::Tensor &v, int64_t n_v, int64_t dim, double reg, at::Tensor gram, const OT &workspace) {
    TORCH_CHECK(dim >= 1 && dim <= 256, "factor_gram_wide: dim must lie in 1..256, got ", dim);
    TORCH_CHECK(n_v >= 0 && n_v <= INT32_MAX, "factor_gram_wide: n_v must lie in 0..2^31-1");
    TORCH_CHECK(v.dim() == 2 && v.size(0) >= n_v && v.size(1) >= dim, "factor_gram_wide: v must be [>= n_v, >= dim]");
    TORCH_CHECK(reg >= 0.0, "factor_gram_wide: reg must be a number >= 0, got ", reg);
    TORCH_CHECK(gram.numel() == dim * dim, "factor_gram_wide: gram must be [dim, dim]");
    const size_t need = RTREC_FACTOR_GRAM_WORKSPACE_BYTES(n_v, dim);
    const size_t ws_bytes = has(workspace) ? static_cast<size_t>(workspace->numel()) * workspace->element_size() : 0;
    TORCH_CHECK(ws_bytes >= need, "factor_gram_wide: the workspace holds ", ws_bytes, " bytes, RTREC_FACTOR_GRAM_WORKSPACE_BYTES(n_v, dim) = ", need);
    one_device("factor_gram_wide", gram, {&v}, {&workspace});
    check(abi().factor_gram_wide(static_cast<int32_t>(n_v), cptr<const float>(v), v.size(1), static_cast<int32_t>(dim),
                                 static_cast<float>(reg), cptr<float>(gram), cptr<void>(workspace), ws_bytes, stream_of(gram)),
          "rtrec_factor_gram_wide");
}

// factor_als_solve's arguments, plus the number of conjugate-gradient steps, whether `out` holds the start vectors, and rs
// [n_jobs] float32 (absent: not wanted): the last squared residual norm per job (include/rtrec_amd_ext.h, "FACTOR ALS CG").
void factor_als_cg(const OT &job_rows, int64_t n_jobs, const at::Tensor &r_ptr, const at::Tensor &r_idx, const at::Tensor &r_val,
                   const at::Tensor &v, int64_t n_v, int64_t dim, const at::Tensor &gram, double alpha, int64_t cg_steps,
                   bool warm_start, at::Tensor out, at::Tensor status, const OT &rs) {
    TORCH_CHECK(dim >= 1 && dim <= 256, "factor_als_cg: dim must lie in 1..256, got ", dim);
    TORCH_CHECK(cg_steps >= 1 && cg_steps <= 64, "factor_als_cg: cg_steps must lie in 1..64, got ", cg_steps);
    TORCH_CHECK(n_jobs >= 0 && n_jobs <= INT32_MAX && n_v >= 0 && n_v <= INT32_MAX, "factor_als_cg: n_jobs and n_v must lie in 0..2^31-1");
    TORCH_CHECK(r_ptr.numel() >= 1 && r_ptr.numel() - 1 <= INT32_MAX, "factor_als_cg: r_ptr must hold n_rows + 1 offsets");
    const int64_t n_rows = r_ptr.numel() - 1;
    TORCH_CHECK(r_val.numel() == r_idx.numel(), "factor_als_cg: r_val must hold one value per entry of r_idx");
    TORCH_CHECK(v.dim() == 2 && v.size(0) >= n_v && v.size(1) >= dim, "factor_als_cg: v must be [>= n_v, >= dim]");
    TORCH_CHECK(gram.numel() == dim * dim, "factor_als_cg: gram must be [dim, dim]");
    TORCH_CHECK(alpha > 0.0, "factor_als_cg: alpha must be a number > 0, got ", alpha);
    TORCH_CHECK(out.dim() == 2 && out.size(0) >= n_rows && out.size(1) >= dim, "factor_als_cg: out must be [>= n_rows, >= dim]");
    TORCH_CHECK(!has(job_rows) || job_rows->numel() == n_jobs, "factor_als_cg: job_rows must hold one entry per job");
    TORCH_CHECK(has(job_rows) || n_jobs <= n_rows, "factor_als_cg: without job_rows there is at most one job per row");
    TORCH_CHECK(status.numel() >= n_jobs && (status.scalar_type() == at::kByte || status.scalar_type() == at::kBool),
                "factor_als_cg: status must hold one uint8 / bool entry per job");
    TORCH_CHECK(!has(rs) || rs->numel() >= n_jobs, "factor_als_cg: rs must hold one float32 entry per job");
    one_device("factor_als_cg", out, {&r_ptr, &r_idx, &r_val, &v, &gram, &status}, {&job_rows, &rs});
    check(abi().factor_als_cg(static_cast<int32_t>(n_jobs), cptr<const int32_t>(job_rows), static_cast<int32_t>(n_rows),
                              cptr<const int32_t>(r_ptr), cptr<const int32_t>(r_idx), cptr<const float>(r_val), r_idx.numel(),
                              cptr<const float>(v), v.size(1), static_cast<int32_t>(n_v), static_cast<int32_t>(dim),
                              cptr<const float>(gram), static_cast<float>(alpha), static_cast<int32_t>(cg_steps), warm_start ? 1 : 0,
                              cptr<float>(out), out.size(1), static_cast<uint8_t *>(cptr<void>(status)), cptr<float>(rs),
                              stream_of(out)),
          "rtrec_factor_als_cg");
}

}  // namespace

// Bind the ops to a build of the C-ABI library (called once by rtrec_amd.ops with _native.lib_path()).
extern "C" int rtrec_ops_bind(const char *path) {
    try {
        void *h = dlopen(path, RTLD_NOW | RTLD_GLOBAL);
        if (!h) return -1;
        Abi a;
        a.handle = h;
        bind_one(h, a.last_error, "rtrec_amd_last_error");
        bind_one(h, a.column_sqnorms, "rtrec_slim_column_sqnorms");
        bind_one(h, a.fit_workspace_init, "rtrec_slim_fit_workspace_init");
        bind_one(h, a.gram_matrix, "rtrec_slim_gram_matrix");
        bind_one(h, a.fit_columns_opt, "rtrec_slim_fit_columns_opt");
        bind_one(h, a.score_topk_opt, "rtrec_slim_score_topk_opt");
        bind_one(h, a.score_rows, "rtrec_slim_score_rows");
        bind_one(h, a.merge_topk_strided, "rtrec_slim_merge_topk_strided");
        bind_one(h, a.similar_topk, "rtrec_slim_similar_topk");
        bind_one(h, a.store_decay_device, "rtrec_store_decay_device");
        bind_one(h, a.store_fold_device, "rtrec_store_fold_device");
        bind_one(h, a.fit_sgd_epochs, "rtrec_slim_fit_sgd_epochs");
        bind_one(h, a.first_touch_aux, "rtrec_slim_first_touch_aux");
        bind_one(h, a.dense_fill, "rtrec_slim_dense_fill");
        bind_one(h, a.refine_topk_f64, "rtrec_slim_refine_topk_f64");
        bind_one(h, a.score_candidates, "rtrec_slim_score_candidates");
        bind_one(h, a.seg_plan, "rtrec_slim_seg_plan");
        bind_one(h, a.seg_fill, "rtrec_slim_seg_fill");
        bind_one(h, a.ordered_sums, "rtrec_slim_ordered_sums");
        bind_one(h, a.rank_metrics, "rtrec_rank_metrics");
        bind_one(h, a.explain_topk, "rtrec_slim_explain_topk");
        bind_one(h, a.audience_topk, "rtrec_slim_audience_topk");
        bind_one(h, a.score_pairs, "rtrec_slim_score_pairs");
        bind_one(h, a.diversify_lists, "rtrec_slim_diversify_lists");
        bind_one(h, a.list_quality, "rtrec_slim_list_quality");
        bind_one(h, a.catalogue_ranks, "rtrec_slim_catalogue_ranks");
        bind_one(h, a.blend_lists, "rtrec_slim_blend_lists");
        bind_one(h, a.factor_topk, "rtrec_factor_topk");
        bind_one(h, a.feature_repr, "rtrec_feature_repr");
        bind_one(h, a.factor_norms, "rtrec_factor_norms");
        bind_one(h, a.factor_similar_topk, "rtrec_factor_similar_topk");
        bind_one(h, a.similar_blend, "rtrec_similar_blend");
        bind_one(h, a.factor_gram, "rtrec_factor_gram");
        bind_one(h, a.factor_als_solve, "rtrec_factor_als_solve");
        bind_one(h, a.factor_gram_wide, "rtrec_factor_gram_wide");
        bind_one(h, a.factor_als_cg, "rtrec_factor_als_cg");
        g_abi = a;
        return 0;
    } catch (const std::exception &) {
        return -2;
    }
}

TORCH_LIBRARY(rtrec_amd, m) {
    m.def("column_sqnorms(Tensor cptr, Tensor cval, Tensor(a!) out) -> ()");
    m.def("fit_workspace_init(Tensor(a!) ws, int n_users, int n_items, int n_slots, int top_features) -> ()");
    m.def("gram_matrix(Tensor cptr, Tensor crow, Tensor cval, Tensor top_items, Tensor(a!) ws, Tensor(b!) gram, int n_users, int n_items) -> ()");
    m.def("fit_columns(Tensor cptr, Tensor crow, Tensor cval, Tensor rptr, Tensor rcol, Tensor rval, Tensor sqn, Tensor targets, "
          "int n_users, int n_items, float l1_reg, float l2_reg, float tol, int max_iter, int seed, bool positive, int top_features, "
          "Tensor(a!) out_items, Tensor(b!) out_coef, Tensor(c!) out_count, Tensor(d!) out_n_iter, int cap, Tensor(e!) ws, int n_slots, "
          "Tensor(f!) queue, Tensor(g!)? trace, Tensor? gram, Tensor? gram_index, int gram_n, float gram_rel_err, int fast, int kernel, "
          "int colwalk_min_rows, int screen_min, int lane_max, Tensor(h!)? xty_ws, Tensor? col_order, int fold) -> ()");
    m.def("score_topk(Tensor? row_ids, Tensor xb_ptr, Tensor xb_col, Tensor xb_val, int n_rows, int n_items, int n_cols, int col_offset, "
          "Tensor? col_ids, Tensor? col_map, int tile_cols, int n_tiles, Tensor? tile_ptr, Tensor? w_col, Tensor? w_val, Tensor? dense_idx, "
          "Tensor? dense_val, Tensor? row_hdr, Tensor? col_rank, int top_k, bool filter_interacted, int mode, bool acc_f64, "
          "Tensor(a!) ids, Tensor(b!) scores, Tensor(c!)? scores64, Tensor(d!) aux, Tensor(e!) count, Tensor(f!) ws, Tensor? fr_map, "
          "Tensor? fr_col_ids, Tensor? fr_col_map, Tensor? fr_w, Tensor? fr_tile_rows, Tensor? fr_tile_off, Tensor? fr_super_kb, "
          "Tensor? fr_super_tile, Tensor? fr_frag_tile, int fr_rows, int fr_tile_cols, int fr_n_tiles, int fr_n_frags, int fr_n_super, "
          "int fr_buf_bytes, Tensor(g!)? fr_scratch, Tensor? row_order, int timer, int diagnostics, Tensor(h!)? rescored, "
          "int row_order_grouped, Tensor? sg_info, Tensor? sg_ptr, Tensor? sg_ent, Tensor? sg_bound, Tensor? sg_col_ids, int sg_tile_cols, "
          "int sg_n_tiles, int sg_rows, int sg_n_cols, Tensor? sg_trow_ptr, Tensor? sg_trow, Tensor(i!)? sg_scratch, "
          "Tensor(j!)? flagged, int aux_stream) -> ()");
    m.def("score_rows(Tensor? row_ids, Tensor xb_ptr, Tensor xb_col, Tensor xb_val, int n_rows, int n_items, int n_cols, int col_offset, "
          "int tile_cols, int n_tiles, Tensor tile_ptr, Tensor w_col, Tensor w_val, bool acc_f64, Tensor(a!) out) -> ()");
    m.def("merge_topk(Tensor in_ids, Tensor in_scores, Tensor? in_scores64, Tensor in_aux, Tensor in_count, int top_k, "
          "Tensor(a!) out_ids, Tensor(b!) out_scores, Tensor(c!) out_count) -> ()");
    m.def("similar_topk(Tensor queries, Tensor wc_ptr, Tensor wc_row, Tensor wc_val, int top_k, Tensor(a!) ids, Tensor(b!) scores, "
          "Tensor(c!) count) -> ()");
    m.def("store_decay_device(Tensor raw, Tensor ts, float rate, float now, Tensor(a!) out, Tensor(b!) unsafe_idx, Tensor(c!) unsafe_count) -> ()");
    m.def("store_fold_device(Tensor order, Tensor start, Tensor delta, Tensor tstamp, Tensor? old, float lo, float hi, bool upsert, "
          "Tensor(a!) out_val, Tensor(b!) out_ts, Tensor(c!) out_val32) -> ()");
    m.def("fit_sgd_epochs(Tensor cptr, Tensor ttime, Tensor tval, Tensor targets, Tensor sel, Tensor sel_count, int n_users, int n_items, "
          "int nnz, int cap, int first_epoch, int n_epochs, int max_iter, float tol, Tensor eta, Tensor ws_before, Tensor ws_after, "
          "Tensor u_after, Tensor reset_cnt, Tensor reset_mult, Tensor(a!) w, Tensor(b!) q, Tensor(c!) best_loss, Tensor(d!) no_improve, "
          "Tensor(e!) n_iter, Tensor(f!) unfinished) -> ()");
    m.def("first_touch_aux(Tensor? row_ids, Tensor xb_ptr, Tensor xb_col, int n_rows, int n_items, Tensor wc_ptr, Tensor wc_row, int top_k, "
          "Tensor ids, Tensor count, Tensor(a!) aux) -> ()");
    m.def("dense_fill(Tensor? row_ids, Tensor xb_ptr, Tensor xb_col, int n_rows, int col_lo, int col_hi, int top_k, bool filter_interacted, "
          "Tensor(a!) ids, Tensor(b!) scores, Tensor(c!) aux, Tensor(d!) count, Tensor flagged_in, Tensor(e!) flagged_out) -> ()");
    m.def("refine_topk_f64(Tensor? row_ids, Tensor xb_ptr, Tensor xb_col, Tensor xb_val, int n_rows, int n_items, Tensor wc_ptr, "
          "Tensor wc_row, Tensor wc_val, int top_k, Tensor in_ids, Tensor in_scores, Tensor in_count, float rel_margin, Tensor? abs_slack, "
          "Tensor(a!) out_ids, Tensor(b!) out_scores, Tensor(c!) out_scores64, Tensor(d!) out_count, Tensor(e!) flagged) -> ()");
    m.def("score_candidates(Tensor? row_ids, Tensor xb_ptr, Tensor xb_col, Tensor xb_val, int n_rows, int n_items, Tensor wc_ptr, "
          "Tensor wc_row, Tensor wc_val, Tensor cands, int top_k, bool acc_f64, Tensor(a!) ids, Tensor(b!) scores, Tensor(c!)? scores64, "
          "Tensor(d!) count) -> ()");
    m.def("seg_plan(Tensor rows, Tensor cols, int n_items, int col_lo, int col_hi, Tensor labels, Tensor(a!) ws) -> int[]");
    m.def("seg_fill(Tensor rows, Tensor cols, Tensor vals, int n_items, int col_lo, int col_hi, Tensor plan_ws, int n_cols, int n_rows, "
          "int tile_cols, int n_tiles, Tensor(a!) ws, Tensor(b!) info, Tensor(c!) seg_ptr, Tensor(d!) ent, Tensor(e!) bound, "
          "Tensor(f!) col_ids, Tensor(g!) trow_ptr, Tensor(h!) trow) -> ()");
    m.def("ordered_sums(Tensor values, Tensor offsets, int mode, Tensor(a!) out) -> ()");
    m.def("rank_metrics(Tensor ids, Tensor counts, Tensor truth_ptr, Tensor truth_items, Tensor truth_len, Tensor discount, Tensor ideal, "
          "int size, Tensor(a!) metrics, Tensor(b!) tp, Tensor(c!) rel) -> ()");
    m.def("explain_topk(Tensor? row_ids, Tensor xb_ptr, Tensor xb_col, Tensor xb_val, int n_items, Tensor wc_ptr, Tensor wc_row, "
          "Tensor wc_val, Tensor ids, Tensor counts, int list_k, int top_m, Tensor(a!) items, Tensor(b!) contrib, Tensor(c!) support) -> ()");
    m.def("audience_topk(Tensor items, int n_users, Tensor xc_ptr, Tensor xc_row, Tensor xc_val, Tensor wc_ptr, Tensor wc_row, "
          "Tensor wc_val, int top_n, bool filter_interacted, Tensor? user_mask, Tensor(a!) users, Tensor(b!) scores, "
          "Tensor(c!) count, Tensor(d!) eligible, Tensor(e!) ws) -> ()");
    m.def("score_pairs(Tensor? row_ids, Tensor xb_ptr, Tensor xb_col, Tensor xb_val, int n_items, Tensor wc_ptr, Tensor wc_row, "
          "Tensor wc_val, Tensor ids, Tensor counts, int list_k, int top_k, bool filter_interacted, int waves_per_row, "
          "Tensor(a!) scores, Tensor(b!) support, Tensor(c!) order, Tensor(d!) count) -> ()");
    // the extension surface (include/rtrec_amd_ext.h)
    m.def("diversify_lists(Tensor wc_ptr, Tensor wc_row, Tensor wc_val, int n_items, Tensor ids, Tensor scores, Tensor counts, int list_k, "
          "int keep, float lam, int waves_per_row, Tensor(a!) order, Tensor(b!) value, Tensor(c!) penalty, Tensor(d!) count) -> ()");
    m.def("list_quality(Tensor wc_ptr, Tensor wc_row, Tensor wc_val, int n_items, Tensor ids, Tensor counts, int list_k, Tensor? item_weight, "
          "int waves_per_row, Tensor(a!) n, Tensor(b!) sim_sum, Tensor(c!) linked, Tensor(d!) weight_sum, Tensor(e!)? exposure) -> ()");
    m.def("catalogue_ranks(Tensor scores, int n_items, Tensor? row_ids, Tensor xb_ptr, Tensor xb_col, bool filter_interacted, int mode, "
          "Tensor tg_ptr, Tensor tg_items, Tensor(a!) above, Tensor(b!) tied, Tensor(c!) score, Tensor(d!) competing) -> ()");
    m.def("blend_lists(int n_items, Tensor a_ids, Tensor a_scores, Tensor a_counts, int ka, Tensor b_ids, Tensor b_scores, Tensor b_counts, "
          "int kb, int keep, float weight_b, bool contacts, float k, bool mnz, Tensor? row_ids, Tensor? xb_ptr, Tensor? xb_col, "
          "Tensor? cn_ptr, Tensor? cn_col, Tensor? cn_val, int waves_per_row, Tensor(a!) ids, Tensor(b!) value, Tensor(c!) source, "
          "Tensor(d!) count) -> ()");
    m.def("factor_topk(Tensor? row_ids, Tensor? p_index, int n_x_rows, Tensor p, Tensor qt, int n_items, int dim, Tensor? item_mask, "
          "Tensor? xb_ptr, Tensor? xb_col, bool filter_interacted, int top_k, int item_splits, Tensor(a!) ids, Tensor(b!) scores, "
          "Tensor(c!) count, Tensor(d!)? workspace) -> ()");
    m.def("feature_repr(Tensor? job_rows, Tensor f_ptr, Tensor f_col, Tensor? f_val, Tensor e, int dim_e, Tensor? bias, int layout, "
          "int n_jobs, Tensor(a!) out, int row_stride, int comp_stride, Tensor(b!)? has) -> ()");
    m.def("factor_norms(Tensor v, int n, int dim, int row_stride, int comp_stride, Tensor(a!) out) -> ()");
    m.def("factor_similar_topk(Tensor? queries, Tensor? p, Tensor? p_norms, Tensor qt, int n_items, int dim, Tensor norms, "
          "Tensor? item_mask, int top_k, int item_splits, bool write_cosine, Tensor(a!) ids, Tensor(b!) scores, Tensor(c!) count, "
          "Tensor(d!)? div, Tensor(e!)? workspace) -> ()");
    m.def("similar_blend(int n_items, Tensor a_ids, Tensor a_scores, Tensor a_counts, int ka, Tensor? a_div, Tensor b_ids, "
          "Tensor b_scores, Tensor b_counts, int kb, Tensor? exclude, int keep, int waves_per_row, Tensor(a!) ids, Tensor(b!) value, "
          "Tensor(c!) source, Tensor(d!) count) -> ()");
    m.def("factor_gram(Tensor v, int n_v, int dim, float reg, Tensor(a!) gram, Tensor(b!)? workspace) -> ()");
    m.def("factor_als_solve(Tensor? job_rows, int n_jobs, Tensor r_ptr, Tensor r_idx, Tensor r_val, Tensor v, int n_v, int dim, "
          "Tensor gram, float alpha, Tensor(a!) out, Tensor(b!) status) -> ()");
    m.def("factor_gram_wide(Tensor v, int n_v, int dim, float reg, Tensor(a!) gram, Tensor(b!)? workspace) -> ()");
    m.def("factor_als_cg(Tensor? job_rows, int n_jobs, Tensor r_ptr, Tensor r_idx, Tensor r_val, Tensor v, int n_v, int dim, "
          "Tensor gram, float alpha, int cg_steps, bool warm_start, Tensor(a!) out, Tensor(b!) status, Tensor(c!)? rs) -> ()");
}

TORCH_LIBRARY_IMPL(rtrec_amd, CUDA, m) {
    m.impl("column_sqnorms", &column_sqnorms);
    m.impl("fit_workspace_init", &fit_workspace_init);
    m.impl("gram_matrix", &gram_matrix);
    m.impl("fit_columns", &fit_columns);
    m.impl("score_topk", &score_topk);
    m.impl("score_rows", &score_rows);
    m.impl("merge_topk", &merge_topk);
    m.impl("similar_topk", &similar_topk);
    m.impl("store_decay_device", &store_decay_device);
    m.impl("store_fold_device", &store_fold_device);
    m.impl("fit_sgd_epochs", &fit_sgd_epochs);
    m.impl("first_touch_aux", &first_touch_aux);
    m.impl("dense_fill", &dense_fill);
    m.impl("refine_topk_f64", &refine_topk_f64);
    m.impl("score_candidates", &score_candidates);
    m.impl("seg_plan", &seg_plan);
    m.impl("seg_fill", &seg_fill);
    m.impl("ordered_sums", &ordered_sums);
    m.impl("rank_metrics", &rank_metrics);
    m.impl("explain_topk", &explain_topk);
    m.impl("audience_topk", &audience_topk);
    m.impl("score_pairs", &score_pairs);
    m.impl("diversify_lists", &diversify_lists);
    m.impl("list_quality", &list_quality);
    m.impl("catalogue_ranks", &catalogue_ranks);
    m.impl("blend_lists", &blend_lists);
    m.impl("factor_topk", &factor_topk);
    m.impl("feature_repr", &feature_repr);
    m.impl("factor_norms", &factor_norms);
    m.impl("factor_similar_topk", &factor_similar_topk);
    m.impl("similar_blend", &similar_blend);
    m.impl("factor_gram", &factor_gram);
    m.impl("factor_als_solve", &factor_als_solve);
    m.impl("factor_gram_wide", &factor_gram_wide);
    m.impl("factor_als_cg", &factor_als_cg);
}
