// MeshAnything inference engine for MI355X (gfx950): the C ABI (include/meshanything_amd.h) -- thin wrappers that check their pointers and call into
// the host headers engine_*.hpp (this stays the library's one translation unit).
//
// Phases (reference: MeshAnything.forward, MeshAnything/models/meshanything.py:134-176):
//   encode      point cloud -> 257x768 latents -> 257x1024 prefix        (MFMA GEMMs + LDS-tiled attention)
//   prefill     24 OPT layers over the prefix, fills the KV cache        (same kernels, causal)
//   decode      <= 7201 steps, each = 51 launches (batch 1: embed + 24 x [q/k/v + attention | out_proj + fc1 + fc2] + lm_head
//               + pick) replayed from ONE hipGraph per batch size; all step-varying scalars live in per-row device DecState
//               records, so the graph never changes.  Batches of >= 4 rows (bf16) run the layers as skinny MFMA GEMMs.
//   detokenize  codebook gather + 6 BERT layers over 1057 tokens + per-coordinate argmax
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <dlfcn.h>
#include <exception>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/meshanything_amd.h"
#include "attn.hpp"
#include "attn2.hpp"
#include "attn_decode.hpp"
#include "common.hpp"
#include "dense_ops.hpp"
#include "gemm.hpp"
#include "gemm_decode.hpp"
#include "gemm_tile.hpp"
#include "gemm256.hpp"
#include "gemv.hpp"
#include "misc.hpp"
#include "oproj_fc1.hpp"
#include "qkv_attn.hpp"
#include "rows_attn.hpp"
#include "rows_mlp.hpp"
#include "state.hpp"
#include "surface_sample.hpp"
#include "watertight.hpp"
#include "mesh_normals.hpp"
#include "mesh_fit.hpp"
#include "mesh_score.hpp"
#include "pc_normals.hpp"
#include "pc_fps.hpp"
#include "pc_grid.hpp"
#include "pc_radius.hpp"
#include "pc_cluster.hpp"
#include "pc_smooth.hpp"
#include "pc_upsample.hpp"
#include "pc_align.hpp"
#include "pc_plane.hpp"
#include "pc_voxel.hpp"
#include "pc_register.hpp"
#include "pc_coarse.hpp"
// MA_EXPERIMENTAL (build.py: MA_EXPERIMENTAL=1): the measured-and-rejected decode-step forms -- the persistent one-launch step
// (persist.hpp), the rows-looped two-launch layer (rows_fused.hpp) and the layer-pair launch (layer_fused.hpp); DESIGN.md records why
// each lost.  They are evidence, not product: the shipped library does not contain them, their tests skip without the flag.
#ifdef MA_EXPERIMENTAL
#include "experimental/persist.hpp"
#include "experimental/rows_fused.hpp"
#include "experimental/layer_fused.hpp"
#endif
#include "weights.hpp"

using namespace ma;

// the host side, by phase (the kernels' headers above keep their order: it fixes the order of the kernel instantiations in the code object)
#include "engine_state.hpp"
#include "engine_decode.hpp"
#include "engine_dense.hpp"
#include "engine_generate.hpp"
#include "engine_build.hpp"
#include "engine_options.hpp"

// ================================================================================================ C ABI
extern "C" {

// MA_SRC_HASH: SHA-256 over the sources and flags this library was compiled from (meshanything_amd/build.py passes it); the loader
// compares it with the tree next to the library, so a stale .so cannot travel to a GPU box unnoticed -- and needs no side file
#ifndef MA_SRC_HASH
#define MA_SRC_HASH "unknown"
#endif
const char* ma_version(void) { return "meshanything_amd 0.1 (gfx950) src=" MA_SRC_HASH; }

const char* ma_last_error(const ma_engine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

int ma_engine_create(ma_engine** out, const ma_config* cfg, int device) {
    if (!out || !cfg) { g_create_error = "null argument"; return MA_ERR_INVALID; }
    *out = nullptr;
    ma_engine* e = nullptr;
    int rc = guarded(nullptr, [&] {
        validate_config(*cfg);
        int ndev = 0;
        HIP_CHECK(hipGetDeviceCount(&ndev));
        if (device < 0 || device >= ndev) throw MaError(MA_ERR_INVALID, "device index out of range (" + std::to_string(ndev) + " visible)");
        HIP_CHECK(hipSetDevice(device));
        e = new ma_engine();
        e->cfg = *cfg; e->device = device;
        build_engine(e);
    });
    if (rc != MA_OK) { if (e) ma_engine_destroy(e); return rc; }
    *out = e;
    return MA_OK;
}

void ma_engine_destroy(ma_engine* e) {
    if (e) destroy_engine(e);
}

int ma_engine_set_option(ma_engine* e, const char* name, int64_t value) {
    if (!e || !name) return MA_ERR_INVALID;
    return guarded(e, [&] { set_option(e, name, value); });
}

int ma_engine_get_option(ma_engine* e, const char* name, int64_t* value) {
    if (!e || !name || !value) return MA_ERR_INVALID;
    return guarded(e, [&] { *value = get_option(e, name); });
}

// Large tensors are uploaded in their STORED dtype and converted into their arena slot on the device (the host-side loop of
// pack_tensor converts ~150 M elements per second on one core: 4.4 s for the 350M checkpoint, against 0.4 s this way; same f2bf
// rounding, same bytes -- tests/test_gpu_model_api.py compares the two arenas).  Returns false when the tensor is not eligible:
// pack_tensor then handles it, including every error message.
static bool load_tensor_on_device(ma_engine* e, const ma_tensor_desc& t) {
    if (!t.name || !t.data || t.ndim < 1 || t.ndim > 3 || t.dtype < MA_DTYPE_F32 || t.dtype > MA_DTYPE_F16) return false;
    bool dropped;
    const Source* s = find_source(e->L, t.name, &dropped);
    if (!s || dropped) return false;
    long long lead = 1;
    for (int i = 0; i + 1 < t.ndim; ++i) lead *= t.shape[i];
    if (lead != s->src_rows || t.shape[t.ndim - 1] != s->src_cols) return false;
    const size_t elems = (size_t)s->take_rows * s->take_cols;
    if (elems < (1u << 16)) return false;
    const Entry& en = e->L.entries[s->entry];
    const size_t src_esz = t.dtype == MA_DTYPE_F32 ? 4 : 2, src_bytes = (size_t)s->take_rows * s->src_cols * src_esz;
    if (e->stage_bytes < src_bytes) {
        if (e->stage) (void)hipFree(e->stage);
        e->stage = nullptr; e->stage_bytes = 0;
        HIP_CHECK(hipMalloc(&e->stage, src_bytes));
        e->stage_bytes = src_bytes;
    }
    // the previous tensor's conversion kernel reads this staging buffer: wait for it explicitly (the implicit ordering of a pageable
    // copy behind kernels holds on the legacy null stream only, not under -fgpu-default-stream=per-thread)
    HIP_CHECK(hipStreamSynchronize(nullptr));
    HIP_CHECK(hipMemcpy(e->stage, t.data, src_bytes, hipMemcpyHostToDevice));
    const int esz = en.dtype == MA_DTYPE_F32 ? 4 : 2;
    void* dst = e->arena + en.offset + s->dst_elem * esz;
    const int blocks = (int)std::min<size_t>((elems + 255) / 256, 65535u * 16u);
    hipLaunchKernelGGL(cvt_weight_kernel, dim3(blocks), dim3(256), 0, nullptr, e->stage, t.dtype, s->src_cols, dst, en.dtype, en.cols, s->take_rows, s->take_cols);
    HIP_CHECK(hipGetLastError());
    e->ps.filled[s->entry] += elems;
    return true;
}

int ma_engine_load_weights(ma_engine* e, const ma_tensor_desc* tensors, int n) {
    if (!e || (!tensors && n > 0)) return MA_ERR_INVALID;
    return guarded(e, [&] {
        for (int i = 0; i < n; ++i) {
            if (load_tensor_on_device(e, tensors[i])) continue;
            std::string err;
            int rc = pack_tensor(e->L, e->ps, tensors[i], err, [&](size_t off, const void* p, size_t nb) {
                HIP_CHECK(hipMemcpy(e->arena + off, p, nb, hipMemcpyHostToDevice));
            });
            if (rc != MA_OK) throw MaError(rc, err);
        }
    });
}

int ma_engine_finalize_weights(ma_engine* e) {
    if (!e) return MA_ERR_INVALID;
    return guarded(e, [&] {
        std::string missing;
        if (!pack_complete(e->L, e->ps, missing)) throw MaError(MA_ERR_MISSING, "checkpoint incomplete, missing: " + missing);
        HIP_CHECK(hipDeviceSynchronize());                   // the device-side conversions of the last tensors
        if (e->stage) { (void)hipFree(e->stage); e->stage = nullptr; e->stage_bytes = 0; }
        e->weights_ready = true; e->embtab_ready = false;
    });
}

int ma_engine_arena(ma_engine* e, void** dev_ptr, size_t* bytes) {
    if (!e || !dev_ptr || !bytes) return MA_ERR_INVALID;
    *dev_ptr = e->arena; *bytes = e->L.bytes;
    return MA_OK;
}

int ma_engine_mark_weights_loaded(ma_engine* e) {
    if (!e) return MA_ERR_INVALID;
    e->weights_ready = true; e->embtab_ready = false;
    return MA_OK;
}

int ma_engine_broadcast_weights(ma_engine* e, void* nccl_comm, int root, void* stream) {
    if (!e || !nccl_comm) return MA_ERR_INVALID;
    return guarded(e, [&] {
        // RCCL is resolved lazily so that the library loads on hosts without librccl (CPU-only checks)
        typedef int (*bcast_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
        static bcast_fn fn = nullptr;
        if (!fn) {
            void* h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
            if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
            if (!h) throw MaError(MA_ERR_NCCL, std::string("cannot load librccl.so: ") + dlerror());
            fn = reinterpret_cast<bcast_fn>(dlsym(h, "ncclBroadcast"));
            if (!fn) throw MaError(MA_ERR_NCCL, "ncclBroadcast not found in librccl.so");
        }
        const int rc = fn(e->arena, e->arena, e->L.bytes, /*ncclInt8*/ 0, root, nccl_comm, reinterpret_cast<hipStream_t>(stream));
        if (rc != 0) throw MaError(MA_ERR_NCCL, "ncclBroadcast failed with code " + std::to_string(rc));
        e->weights_ready = true; e->embtab_ready = false;
    });
}

// ---- host-only arena description / packing ------------------------------------------------------------------------
static int layout_for(const ma_config* cfg, Layout& L, std::string& err) {
    try { validate_config(*cfg); L = build_layout(*cfg); return MA_OK; }
    catch (const MaError& x) { err = x.msg; return x.code; }
    catch (const std::exception& x) { err = x.what(); return MA_ERR_INVALID; }
}
static int layout_for(const ma_config* cfg, Layout& L) {      // ... for the entry points that report through ma_last_error(NULL)
    if (!cfg) return MA_ERR_INVALID;
    return layout_for(cfg, L, g_create_error);
}

int64_t ma_arena_bytes(const ma_config* cfg) {
    Layout L;
    const int rc = layout_for(cfg, L);
    return rc != MA_OK ? rc : (int64_t)L.bytes;
}

int ma_arena_num_entries(const ma_config* cfg) {
    Layout L;
    const int rc = layout_for(cfg, L);
    return rc != MA_OK ? rc : (int)L.entries.size();
}

int ma_arena_entry(const ma_config* cfg, int i, char* name, int name_cap, int64_t* offset, int64_t* bytes, int32_t* dtype, int32_t* rows, int32_t* cols) {
    Layout L;
    const int rc = layout_for(cfg, L);
    if (rc != MA_OK) return rc;
    if (i < 0 || i >= (int)L.entries.size()) return MA_ERR_INVALID;
    const Entry& en = L.entries[i];
    if (name && name_cap > 0) { snprintf(name, name_cap, "%s", en.name.c_str()); }
    if (offset) *offset = (int64_t)en.offset;
    if (bytes) *bytes = (int64_t)en.bytes;
    if (dtype) *dtype = en.dtype;
    if (rows) *rows = en.rows;
    if (cols) *cols = en.cols;
    return MA_OK;
}

int ma_pack_weights_host(const ma_config* cfg, const ma_tensor_desc* tensors, int n, void* host_arena, char* err, int err_cap) {
    auto fail = [&](int code, const std::string& m) { if (err && err_cap > 0) snprintf(err, err_cap, "%s", m.c_str()); return code; };
    if (!cfg || !host_arena || (!tensors && n > 0)) return fail(MA_ERR_INVALID, "null argument");
    Layout L; std::string e;
    int rc = layout_for(cfg, L, e);
    if (rc != MA_OK) return fail(rc, e);
    PackState ps; pack_state_init(L, ps);
    std::memset(host_arena, 0, L.bytes);
    for (int i = 0; i < n; ++i) {
        rc = pack_tensor(L, ps, tensors[i], e, [&](size_t off, const void* p, size_t nb) { std::memcpy(reinterpret_cast<char*>(host_arena) + off, p, nb); });
        if (rc != MA_OK) return fail(rc, e);
    }
    std::string missing;
    if (!pack_complete(L, ps, missing)) return fail(MA_ERR_MISSING, "checkpoint incomplete, missing: " + missing);
    return MA_OK;
}

int ma_engine_upload_arena(ma_engine* e, const void* host_arena, size_t bytes) {
    if (!e || !host_arena) return MA_ERR_INVALID;
    return guarded(e, [&] {
        if (bytes != e->L.bytes) throw MaError(MA_ERR_SHAPE, "arena size mismatch");
        HIP_CHECK(hipMemcpy(e->arena, host_arena, bytes, hipMemcpyHostToDevice));
        e->weights_ready = true; e->embtab_ready = false;
    });
}

// ---- hot path ------------------------------------------------------------------------------------------------------
int ma_encode(ma_engine* e, const void* pc, int pc_dtype, int B, float* latents, float* prefix, void* stream) {
    if (!e || !pc || !latents) return MA_ERR_INVALID;
    return guarded(e, [&] {
        require_ready(e); check_batch(e, B);
        if (pc_dtype != MA_DTYPE_F32 && pc_dtype != MA_DTYPE_F16) throw MaError(MA_ERR_INVALID, "pc_dtype must be F32 or F16");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        RoctxRange range("ma_encode");
        const Dense enc{e, s, e->bf16 && !e->enc_exact};
        const size_t pstride = (size_t)e->cfg.n_points * 6 * (pc_dtype == MA_DTYPE_F16 ? 2 : 4);
        for (int b0 = 0; b0 < B; b0 += e->dense_rows) {          // the whole chunk goes through every GEMM at once (M = nb x rows)
            const int nb = std::min(e->dense_rows, B - b0);
            float* lat = latents + (size_t)b0 * e->T * e->cfg.enc_width;
            encode_chunk(enc, reinterpret_cast<const char*>(pc) + b0 * pstride, pc_dtype, nb, lat);
            if (prefix) prefix_chunk(enc, lat, prefix + (size_t)b0 * e->T * e->cfg.hidden, nb);
        }
    });
}

int ma_to_shape_latents(ma_engine* e, const float* latents, int B, float* out, void* stream) {
    if (!e || !latents || !out) return MA_ERR_INVALID;
    return guarded(e, [&] {
        require_ready(e); check_batch(e, B);
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        const Dense enc{e, s, e->bf16 && !e->enc_exact};
        const size_t n = (size_t)e->cfg.num_latents * e->cfg.enc_width;
        for (int b0 = 0; b0 < B; b0 += e->dense_rows) {
            const int nb = std::min(e->dense_rows, B - b0);
            shape_latents_chunk(enc, latents + b0 * n, e->cfg.enc_width, RowMap{0, 0, 0}, nb);
            HIP_CHECK(hipMemcpyAsync(out + b0 * n, e->w_lat2, (size_t)nb * n * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
    });
}

int ma_process_point_feature(ma_engine* e, const float* point_feature, int B, float* prefix, void* stream) {
    if (!e || !point_feature || !prefix) return MA_ERR_INVALID;
    return guarded(e, [&] {
        require_ready(e); check_batch(e, B);
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        const Dense enc{e, s, e->bf16 && !e->enc_exact};
        for (int b0 = 0; b0 < B; b0 += e->dense_rows) {
            const int nb = std::min(e->dense_rows, B - b0);
            prefix_chunk(enc, point_feature + (size_t)b0 * e->T * e->cfg.enc_width, prefix + (size_t)b0 * e->T * e->cfg.hidden, nb);
        }
    });
}

int ma_get_codes(ma_engine* e, const int64_t* ids, int B, float* codes, void* stream) {
    if (!e || !ids || !codes) return MA_ERR_INVALID;
    return guarded(e, [&] {
        require_ready(e); check_batch(e, B);
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        const int D = e->cfg.codebook_dim, nf = e->nf;
        for (int b0 = 0; b0 < B; b0 += e->dense_rows) {
            const int nb = std::min(e->dense_rows, B - b0);
            hipLaunchKernelGGL((codes_gather2_kernel<float>), dim3(ceil_div(nb * nf * 3 * (D / 4), 256)), dim3(256), 0, s, reinterpret_cast<const long long*>(ids) + (size_t)b0 * nf * 9,
                               e->dw.codebooks, D, nb * nf, codes + (size_t)b0 * nf * 3 * D, (float*)nullptr, e->w_mask);
            HIP_CHECK(hipGetLastError());
        }
    });
}

int ma_generate(ma_engine* e, const float* prefix, int B, const ma_sample_cfg* sc_in, int64_t* tokens, int32_t* lengths, int32_t* n_generated, void* stream) {
    if (!e || !prefix || !tokens) return MA_ERR_INVALID;
    return guarded(e, [&] {
        require_ready(e); check_batch(e, B);
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        const ma_sample_cfg sc = resolve_sample_cfg(e, sc_in);
        // rows are independent (no cross-batch op anywhere in meshanything.py:134-176) but step together: one weight stream per step
        const int nmax = generate_batch(e, s, prefix, B, sc, reinterpret_cast<long long*>(tokens), lengths);
        HIP_CHECK(hipStreamSynchronize(s));
        if (n_generated) *n_generated = nmax;
    });
}

int ma_postprocess_tokens(ma_engine* e, const int64_t* tokens, int ld_tokens, int B, int n_generated, int64_t* ids, void* stream) {
    if (!e || !tokens || !ids) return MA_ERR_INVALID;
    return guarded(e, [&] {
        check_batch(e, B);
        if (n_generated < 0 || n_generated > e->maxnew) throw MaError(MA_ERR_INVALID, "n_generated out of range [0, 9*n_max_faces+2]");
        if (ld_tokens < n_generated) throw MaError(MA_ERR_INVALID, "ld_tokens smaller than n_generated");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        const int total = B * (e->maxnew - 2);
        hipLaunchKernelGGL(postprocess_tokens_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, s, reinterpret_cast<const long long*>(tokens), ld_tokens,
                           n_generated, e->maxnew, reinterpret_cast<long long*>(ids), B);
        HIP_CHECK(hipGetLastError());
    });
}

int ma_detokenize_embeds(ma_engine* e, const int64_t* ids, const float* codes, const float* latents, int B, float* coords, void* stream) {
    if (!e || !ids || !latents || !coords) return MA_ERR_INVALID;
    return guarded(e, [&] {
        require_ready(e); check_batch(e, B);
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        RoctxRange range("ma_detokenize");
        const size_t nf = e->nf;
        for (int b0 = 0; b0 < B; b0 += e->dense_rows) {
            const int nb = std::min(e->dense_rows, B - b0);
            detok_chunk(Dense{e, s, e->bf16}, reinterpret_cast<const long long*>(ids) + (size_t)b0 * nf * 9, codes ? codes + (size_t)b0 * nf * 3 * e->cfg.codebook_dim : nullptr,
                        latents + (size_t)b0 * e->T * e->cfg.enc_width, coords + (size_t)b0 * nf * 9, nb);
        }
    });
}

int ma_detokenize(ma_engine* e, const int64_t* ids, const float* latents, int B, float* coords, void* stream) {
    return ma_detokenize_embeds(e, ids, nullptr, latents, B, coords, stream);
}

int ma_forward(ma_engine* e, const void* pc, int pc_dtype, int B, const ma_sample_cfg* sc, float* coords, int64_t* tokens, int32_t* lengths,
               int32_t* n_generated, int64_t* ids, float* latents, void* stream) {
    if (!e || !pc || !coords) return MA_ERR_INVALID;
    int rc = guarded(e, [&] { require_ready(e); check_batch(e, B); });
    if (rc != MA_OK) return rc;
    float* lat = latents ? latents : e->w_latents;
    int64_t* tok = tokens ? tokens : reinterpret_cast<int64_t*>(e->w_tokens);
    int64_t* idp = ids ? ids : reinterpret_cast<int64_t*>(e->w_ids);
    int32_t ngen = 0;
    if ((rc = ma_encode(e, pc, pc_dtype, B, lat, e->w_prefix, stream)) != MA_OK) return rc;
    if ((rc = ma_generate(e, e->w_prefix, B, sc, tok, lengths, &ngen, stream)) != MA_OK) return rc;
    if (n_generated) *n_generated = ngen;
    if ((rc = ma_postprocess_tokens(e, tok, e->maxnew, B, ngen, idp, stream)) != MA_OK) return rc;
    if ((rc = ma_detokenize(e, idp, lat, B, coords, stream)) != MA_OK) return rc;
    return guarded(e, [&] { HIP_CHECK(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream))); });
}

// ---- kernel-level entry points -------------------------------------------------------------------------------------
int ma_op_gemv(int wdtype, const void* W, const float* bias, const float* x, const float* ln_g, const float* ln_b, float ln_eps, const float* res,
               float* y, float* xn_out, int N, int K, int act, void* stream) {
    return guarded(nullptr, [&] {
        if (!W || !x || !y || N < 1 || K < 8 || K % 8) throw MaError(MA_ERR_INVALID, "ma_op_gemv: bad arguments");
        GemvArgs a{};
        a.W = W; a.bias = bias; a.x = x; a.ln_g = ln_g; a.ln_b = ln_b; a.ln_eps = ln_eps; a.xn_out = xn_out; a.res = res; a.y = y; a.N = N; a.K = K;
        a.act = act; a.round_x = wdtype != MA_DTYPE_F32; a.epi = EPI_PLAIN;
        if (wdtype != MA_DTYPE_BF16 && wdtype != MA_DTYPE_F16 && wdtype != MA_DTYPE_F32) throw MaError(MA_ERR_INVALID, "ma_op_gemv: wdtype");
        launched(PREC_CALL(wdtype != MA_DTYPE_F32, wdtype, T, launch_gemv<T>(a, reinterpret_cast<hipStream_t>(stream))), "gemv");
    });
}

int ma_op_gemm(int wdtype, int impl, const float* A, int lda, const void* W, const float* bias, const float* R, int ldr, float* C, int ldc, int M, int N,
               int K, int act, void* stream) {
    return guarded(nullptr, [&] {
        if (!A || !W || !C) throw MaError(MA_ERR_INVALID, "ma_op_gemm: null pointer");
        GemmArgs g{A, lda, W, bias, R, ldr, C, ldc, M, N, K, act};
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        hipError_t r;
        if (wdtype == MA_DTYPE_BF16 && impl == 0) {
            // the engine's bf16 GEMM takes bf16 activations (gemm_tile.hpp): round A first, as the producing kernel would have
            bf16_t* Ab = nullptr;
            HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&Ab), (size_t)M * K * sizeof(bf16_t)));
            hipLaunchKernelGGL(f32_to_bf16_rows_kernel, dim3(ceil_div(M * K, 256)), dim3(256), 0, s, A, lda, Ab, K, M, K);
            GemmTArgs t{Ab, K, reinterpret_cast<const bf16_t*>(W), bias, R, ldr, C, ldc, nullptr, 0, M, N, K, act};
            t.xcd_swizzle = 1;
            r = launch_gemm_tile<bf16_t>(t, s);
            (void)hipStreamSynchronize(s);
            (void)hipFree(Ab);
        } else if (wdtype == MA_DTYPE_BF16) r = launch_gemm<bf16_t>(g, 1, s);                 // the scalar cross-check kernel
        else if (wdtype == MA_DTYPE_F32) r = launch_gemm<float>(g, impl, s);
        else throw MaError(MA_ERR_INVALID, "ma_op_gemm: wdtype");
        if (r != hipSuccess) throw MaError(MA_ERR_HIP, std::string("ma_op_gemm: ") + hipGetErrorString(r));
    });
}

// the bf16 policy's dense GEMM on its native operands (gemm_tile.hpp): A (M, lda) bf16, W (N, K) bf16; fp32 output C and / or bf16 output Cb
int ma_op_gemm_bf16(const void* A, int lda, const void* W, const float* bias, const float* R, int ldr, float* C, int ldc, void* Cb, int ldcb, int M, int N,
                    int K, int act, void* stream) {
    return ma_op_gemm_bf16_tuned(A, lda, W, bias, R, ldr, C, ldc, Cb, ldcb, M, N, K, act, GemmTune{}.variant, GemmTune{}.tile256, stream);
}

// ... in one of its A/B forms: what the engine options gemm_variant and gemm256 select, with their range and MA_EXPERIMENTAL checks
int ma_op_gemm_bf16_tuned(const void* A, int lda, const void* W, const float* bias, const float* R, int ldr, float* C, int ldc, void* Cb, int ldcb, int M, int N,
                          int K, int act, int variant, int tile256, void* stream) {
    return guarded(nullptr, [&] {
        if (!A || !W || (!C && !Cb)) throw MaError(MA_ERR_INVALID, "ma_op_gemm_bf16: null pointer");
        check_value(find_option("gemm_variant", true), variant);
        check_value(find_option("gemm256", true), tile256);
        const GemmTune tune{variant, tile256};
        GemmTArgs t{reinterpret_cast<const bf16_t*>(A), lda, reinterpret_cast<const bf16_t*>(W), bias, R, ldr, C, ldc, reinterpret_cast<bf16_t*>(Cb), ldcb, M, N, K, act};
        t.xcd_swizzle = 1;
        static int n_cus = -1;
        if (n_cus < 0) { int dev = 0; hipDeviceProp_t prop; n_cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ? prop.multiProcessorCount : 0; }
        op_launched(H16_CALL(g_op_hdt, HT, launch_gemm_dense<HT>(t, n_cus, reinterpret_cast<hipStream_t>(stream), nullptr, nullptr, nullptr, tune)), "ma_op_gemm_bf16");
    });
}

namespace {
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
void check_row_map(const std::string& op, const char* what, int grp, int gstride, int off) {
    if (grp < 0 || off < 0 || (grp > 0 && gstride < grp)) throw MaError(MA_ERR_INVALID, op + ": " + what + " row map needs grp >= 0, off >= 0 and gstride >= grp");
}
// what ln_rows2_kernel can compute: a lane holds at most 16 float4 chunks of a row, the split input exists for 1024 columns only
void check_ln_shape(const std::string& op, int rows, int D, int parts, int64_t part_stride, int split_rows) {
    if (rows <= 0 || D <= 0) throw MaError(MA_ERR_INVALID, op + ": rows and D must be > 0");
    if (D % 4 != 0 || D > 4096) throw MaError(MA_ERR_INVALID, op + ": D must be a multiple of 4 and at most 4096");
    if (parts != 1 && parts != 2 && parts != 4) throw MaError(MA_ERR_INVALID, op + ": parts must be 1, 2 or 4");
    if (parts > 1 && D != 1024) throw MaError(MA_ERR_INVALID, op + ": a split input needs D == 1024");
    if (parts > 1 && (part_stride <= 0 || part_stride % 4 != 0)) throw MaError(MA_ERR_INVALID, op + ": part_stride must be a positive multiple of 4");
    if (split_rows < 0 || split_rows > rows) throw MaError(MA_ERR_INVALID, op + ": split_rows outside [0, rows]");
}
}  // namespace

int ma_op_layernorm(const float* x, int ldx, const float* g, const float* b, float eps, float* y, int ldy, int rows, int D, void* stream) {
    return guarded(nullptr, [&] {
        if (!x || !g || !b || !y) throw MaError(MA_ERR_INVALID, "ma_op_layernorm: null pointer");
        check_ln_shape("ma_op_layernorm", rows, D, 1, 0, 0);
        if (ldx < D || ldy < D || ldx % 4 || ldy % 4) throw MaError(MA_ERR_INVALID, "ma_op_layernorm: leading dimensions must be multiples of 4 and at least D");
        launch_ln_rows2<float>(x, ldx, RowMap{0, 0, 0}, g, b, eps, y, ldy, (float*)nullptr, 0, RowMap{0, 0, 0}, rows, D, reinterpret_cast<hipStream_t>(stream));
        HIP_CHECK(hipGetLastError());
    });
}

// test aid: launch_ln_rows2 with everything Dense::lnrows can set
int ma_op_ln_rows(const float* x, int ldx, int xin_grp, int xin_gstride, int xin_off, const float* g, const float* b, float eps, float* y32, int ld32, void* act,
                  int lda, int act_dtype, int yout_grp, int yout_gstride, int yout_off, int rows, int D, int parts, int64_t part_stride, int split_rows, void* stream) {
    return guarded(nullptr, [&] {
        const std::string op = "ma_op_ln_rows";
        if (!x || !g || !b || (!y32 && !act)) throw MaError(MA_ERR_INVALID, op + ": null pointer");
        check_ln_shape(op, rows, D, parts, part_stride, split_rows);
        if (act_dtype != 0 && act_dtype != 1) throw MaError(MA_ERR_INVALID, op + ": act_dtype must be 0 (fp32) or 1 (the 16-bit format)");
        if (ldx < D || ldx % 4 || (y32 && (ld32 < D || ld32 % 4)) || (act && (lda < D || lda % 4)))
            throw MaError(MA_ERR_INVALID, op + ": leading dimensions must be multiples of 4 and at least D");
        if (!aligned16(x) || !aligned16(g) || !aligned16(b) || !aligned16(y32) || !aligned16(act)) throw MaError(MA_ERR_INVALID, op + ": arrays must be 16-byte aligned");
        check_row_map(op, "input", xin_grp, xin_gstride, xin_off);
        check_row_map(op, "output", yout_grp, yout_gstride, yout_off);
        const RowMap xin{xin_grp, xin_gstride, xin_off}, yout{yout_grp, yout_gstride, yout_off};
        // (a wave reads its whole row before it writes: in place is safe exactly when a row is written where it was read)
        if (y32 == x && (ld32 != ldx || xin_grp != yout_grp || (xin_grp > 0 && xin_gstride != yout_gstride) || xin_off != yout_off))
            throw MaError(MA_ERR_INVALID, op + ": y32 over x needs the same leading dimension and row map on both sides");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        if (act_dtype == 1) H16_DO(g_op_hdt, HT, launch_ln_rows2<HT>(x, ldx, xin, g, b, eps, y32, ld32, reinterpret_cast<HT*>(act), lda, yout, rows, D, s, parts, (long)part_stride, split_rows));
        else launch_ln_rows2<float>(x, ldx, xin, g, b, eps, y32, ld32, reinterpret_cast<float*>(act), lda, yout, rows, D, s, parts, (long)part_stride, split_rows);
        HIP_CHECK(hipGetLastError());
    });
}

// test aid: launch_gemm_dense / launch_gemm with everything Dense::gemm can set; reports what the dispatcher chose
int ma_op_gemm_dense(ma_gemm_dense_args* a, void* stream) {
    return guarded(nullptr, [&] {
        const std::string op = "ma_op_gemm_dense";
        if (!a) throw MaError(MA_ERR_INVALID, op + ": null arguments");
        if (a->struct_size != (int32_t)sizeof(ma_gemm_dense_args)) throw MaError(MA_ERR_INVALID, op + ": struct_size mismatch");
        a->out_parts = 1; a->out_split_rows = 0; a->out_kv_rows = 0; a->out_rows256 = 0;
        auto bad = [&](const char* what) { throw MaError(MA_ERR_INVALID, op + ": " + what); };
        if (a->precision != 0 && a->precision != 1) bad("precision must be 0 (fp32 kernels) or 1 (16-bit dispatcher)");
        const bool is16 = a->precision == 1;
        if (!a->A || !a->W || (!a->C && !a->Cb)) bad("null pointer");
        if (a->M <= 0 || a->N <= 0 || a->K <= 0 || a->K % 32 != 0) bad("need M, N > 0 and K a positive multiple of 32");
        if (a->act != MA_ACT_NONE && a->act != MA_ACT_RELU && a->act != MA_ACT_GELU) bad("act must be 0, 1 or 2");
        if (a->lda < a->K || a->lda % (is16 ? 8 : 4)) bad("lda must be at least K and a multiple of 8 (16-bit) / 4 (fp32)");
        if (a->C && (a->ldc < a->N || a->ldc % 4)) bad("ldc must be at least N and a multiple of 4");
        if (a->R && (a->ldr < a->N || a->ldr % 4)) bad("ldr must be at least N and a multiple of 4");
        if (a->Cb && (a->ldcb < a->N || a->ldcb % 4)) bad("ldcb must be at least N and a multiple of 4");
        if (!aligned16(a->A) || !aligned16(a->W) || !aligned16(a->bias) || !aligned16(a->R) || !aligned16(a->C) || !aligned16(a->Cb) || !aligned16(a->kv_k) || !aligned16(a->kv_v))
            bad("arrays must be 16-byte aligned");
        check_row_map(op, "output", a->cmap_grp, a->cmap_gstride, a->cmap_off);
        if (a->r_mod < 0) bad("r_mod must be >= 0");
        if (a->part < 0 || a->part > 2) bad("part must be 0, 1 or 2");
        if (a->part != 0 && (a->cmap_grp != 0 || a->r_mod != 0)) bad("a GEMM by row parts takes no row map and no broadcast residual");
        if (a->max_parts < 0 || a->max_parts > 4) bad("max_parts must be in [0, 4]");
        if (a->max_parts >= 2 && (!a->C || a->part_stride <= 0 || a->part_stride % 4 != 0)) bad("a split along K needs the fp32 output and part_stride a positive multiple of 4");
        const bool kv = a->kv_k || a->kv_v;
        if (kv) {
            if (!a->kv_k || !a->kv_v) bad("kv_k and kv_v come together");
            if (a->kv_col0 < 64 || a->kv_col0 % 64 != 0 || a->N != 3 * a->kv_col0) bad("the KV planes need kv_col0 a multiple of 64 and N == 3 * kv_col0");
            if (a->kv_T < 1 || a->kv_max_seq < a->kv_T) bad("the KV planes need 1 <= kv_T <= kv_max_seq");
            if (a->kv_row_stride % 8 != 0 || a->kv_row_stride < (uint64_t)(a->kv_col0 / 64) * (uint64_t)a->kv_max_seq * 64u) bad("kv_row_stride must hold a sample's (heads, kv_max_seq, 64) plane and be a multiple of 8");
            if (!a->Cb) bad("the KV planes need the 16-bit output");
        }
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        if (!is16) {
            if (a->Cb || a->part != 0 || a->max_parts >= 2 || kv) bad("precision 0 has the fp32 output only: no Cb, part, split along K or KV planes");
            if (a->impl != 0 && a->impl != 1) bad("impl must be 0 (MFMA) or 1 (plain)");
            GemmArgs g{};
            g.A = reinterpret_cast<const float*>(a->A); g.lda = a->lda; g.W = a->W; g.bias = a->bias; g.R = a->R; g.ldr = a->ldr; g.C = a->C; g.ldc = a->ldc;
            g.M = a->M; g.N = a->N; g.K = a->K; g.act = a->act; g.r_mod = a->r_mod; g.cmap = RowMap{a->cmap_grp, a->cmap_gstride, a->cmap_off};
            op_launched(launch_gemm<float>(g, a->impl, s), "ma_op_gemm_dense");
            return;
        }
        check_value(find_option("gemm_variant", true), a->variant);
        check_value(find_option("gemm256", true), a->tile256);
        GemmTune tune{};
        tune.variant = a->variant; tune.tile256 = a->tile256;
        GemmTArgs t{};
        t.A = reinterpret_cast<const bf16_t*>(a->A); t.lda = a->lda; t.W = reinterpret_cast<const bf16_t*>(a->W); t.bias = a->bias; t.R = a->R; t.ldr = a->ldr;
        t.C = a->C; t.ldc = a->ldc; t.Cb = reinterpret_cast<bf16_t*>(a->Cb); t.ldcb = a->ldcb; t.M = a->M; t.N = a->N; t.K = a->K; t.act = a->act;
        t.r_mod = a->r_mod; t.cmap = RowMap{a->cmap_grp, a->cmap_gstride, a->cmap_off}; t.xcd_swizzle = 1; t.part = a->part;
        if (kv) { t.kv_k = reinterpret_cast<bf16_t*>(a->kv_k); t.kv_v = reinterpret_cast<bf16_t*>(a->kv_v); t.kv_row_stride = (size_t)a->kv_row_stride; t.kv_max_seq = a->kv_max_seq; t.kv_T = a->kv_T; t.kv_col0 = a->kv_col0; }
        GemmSplitK sk;
        sk.max_parts = std::max(1, (int)a->max_parts); sk.part_stride = (long)a->part_stride;
        static int n_cus = -1;
        if (n_cus < 0) { int dev = 0; hipDeviceProp_t prop; n_cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ? prop.multiProcessorCount : 0; }
        int kv_rows = 0, rows256 = 0;
        op_launched(H16_CALL(g_op_hdt, HT, launch_gemm_dense<HT>(t, n_cus, s, kv ? &kv_rows : nullptr, &sk, nullptr, tune, &rows256)), "ma_op_gemm_dense");
        a->out_parts = sk.parts; a->out_split_rows = sk.rows; a->out_kv_rows = kv_rows; a->out_rows256 = rows256;
    });
}

int ma_op_attention(const float* Q, int q_rs, int q_hs, const float* K, int k_rs, int k_hs, const float* V, int v_rs, int v_hs, float* O, int o_rs, int Sq,
                    int Sk, int H, float scale, int causal_offset, int round_bf16, void* stream) {
    return guarded(nullptr, [&] {
        if (!Q || !K || !V || !O) throw MaError(MA_ERR_INVALID, "ma_op_attention: null pointer");
        AttnArgs a{Q, q_rs, q_hs, K, k_rs, k_hs, V, v_rs, v_hs, O, o_rs, Sq, Sk, H, scale, causal_offset, round_bf16};
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        if (round_bf16 == 4) {                               // bf16 tensors, the engine's default kernel (attn2.hpp): V^T packing + swapped-operand attention
            bf16_t* vt = nullptr;
            HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&vt), attn2_vt_elems(Sk, H, 1) * sizeof(bf16_t)));
            hipError_t r = H16_CALL(g_op_hdt, HT, launch_attention2<HT>(a, vt, s));
            (void)hipStreamSynchronize(s);
            (void)hipFree(vt);
            op_launched(r, "ma_op_attention");
            return;
        }
        HIP_CHECK(launch_attention(a, s));
    });
}

// test aid: launch_attention / launch_attention2 with everything Dense::attention can set
int ma_op_attention_dense(ma_attn_dense_args* a, void* stream) {
    return guarded(nullptr, [&] {
        const std::string op = "ma_op_attention_dense";
        if (!a) throw MaError(MA_ERR_INVALID, op + ": null arguments");
        if (a->struct_size != (int32_t)sizeof(ma_attn_dense_args)) throw MaError(MA_ERR_INVALID, op + ": struct_size mismatch");
        auto bad = [&](const char* what) { throw MaError(MA_ERR_INVALID, op + ": " + what); };
        if (a->kernel != 0 && a->kernel != 3 && a->kernel != 4) bad("kernel must be 0 (fp32), 3 (first-generation MFMA, 16-bit tensors) or 4 (attn2)");
        if (a->kernel == 3 && g_op_hdt != MA_DTYPE_BF16) bad("kernel 3 is bf16 only");
        if (!a->Q || !a->K || !a->V || !a->O) bad("null pointer");
        if (!aligned16(a->Q) || !aligned16(a->K) || !aligned16(a->V) || !aligned16(a->O) || !aligned16(a->vt)) bad("arrays must be 16-byte aligned");
        if (a->Sq <= 0 || a->Sk <= 0 || a->H <= 0 || a->batch <= 0) bad("need Sq, Sk, H, batch > 0");
        if (!(a->scale > 0.f) || !std::isfinite(a->scale)) bad("scale must be positive and finite");
        if (a->Sq > (1 << 24) || a->Sk > (1 << 24) || a->causal_offset > (1 << 24)) bad("Sq, Sk and causal_offset must be at most 2^24");
        if (a->q_rs < 64 || a->k_rs < 64 || a->v_rs < 64 || a->o_rs < 64 || a->q_hs < 0 || a->k_hs < 0 || a->v_hs < 0) bad("row strides must be >= 64, head strides >= 0");
        if (a->H > 1 && (a->q_hs < 64 || a->k_hs < 64 || a->v_hs < 64 || a->o_rs < a->H * 64)) bad("more than one head needs head strides >= 64 and o_rs >= H * 64");
        if (a->batch > 1 && (a->k_bs == 0 || a->v_bs == 0 || a->o_bs == 0)) bad("a batch needs sample strides for K, V and O (only q_bs may be 0)");
        if ((a->q_bs | a->k_bs | a->v_bs | a->o_bs) >> 40) bad("sample strides must be below 2^40 elements");
        if (a->kernel == 4) {
            if (!a->vt) bad("kernel 4 needs the V^T workspace");
            if (a->vt_elems < attn2_vt_elems(a->Sk, a->H, a->batch)) bad("V^T workspace too small (ma_attention_vt_workspace_elems)");
        }
        AttnArgs g{a->Q, a->q_rs, a->q_hs, a->K, a->k_rs, a->k_hs, a->V, a->v_rs, a->v_hs, a->O, a->o_rs, a->Sq, a->Sk, a->H, a->scale, a->causal_offset, a->kernel == 0 ? 0 : 3};
        g.batch = a->batch; g.last_len = a->last_len; g.q_bs = (size_t)a->q_bs; g.k_bs = (size_t)a->k_bs; g.v_bs = (size_t)a->v_bs; g.o_bs = (size_t)a->o_bs;
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        if (a->kernel == 4) op_launched(H16_CALL(g_op_hdt, HT, launch_attention2<HT>(g, reinterpret_cast<bf16_t*>(a->vt), s)), "ma_op_attention_dense");
        else op_launched(launch_attention(g, s), "ma_op_attention_dense");
    });
}

size_t ma_attention_vt_workspace_elems(int Sk, int H, int batch) { return (Sk > 0 && H > 0 && batch > 0) ? attn2_vt_elems(Sk, H, batch) : 0; }

int ma_op_decode_attention(int kvdtype, const float* q, const void* kcache, const void* vcache, int H, int max_seq, int len, float* out,
                           void* workspace, void* stream) {
    return guarded(nullptr, [&] {
        if (!q || !kcache || !vcache || !out || !workspace || H < 1 || len < 1 || len > max_seq) throw MaError(MA_ERR_INVALID, "ma_op_decode_attention: bad arguments");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        float* ws = reinterpret_cast<float*>(workspace);
        if (kvdtype != MA_DTYPE_BF16 && kvdtype != MA_DTYPE_F16 && kvdtype != MA_DTYPE_F32) throw MaError(MA_ERR_INVALID, "ma_op_decode_attention: kvdtype");
        const bool is16 = kvdtype != MA_DTYPE_F32;
        HIP_CHECK(PREC_CALL(is16, kvdtype, T, launch_attn_decode<T>(q, kcache, vcache, H, max_seq, nullptr, len, is16 ? 1 : 0, ws, s)));
        // in the engine the merge of the split partials is the prologue of the out_proj GEMV; here it runs on its own
        hipLaunchKernelGGL(attn_merge_kernel, dim3(ceil_div(H * 16, 256)), dim3(256), 0, s, ws, H, out);
        HIP_CHECK(hipGetLastError());
    });
}

// batched single-query attention, final form (attn_decode_final_kernel): B rows, each its own cache plane, all of length `len`;
// out = bf16 [B][H * 64]
int ma_op_decode_attention_rows(const float* q, const void* kcache, const void* vcache, int H, int max_seq, int len, int B, size_t kv_row_stride,
                                int waves, int halves, void* out, void* stream) {
    return guarded(nullptr, [&] {
        if (!q || !kcache || !vcache || !out || H < 1 || B < 1 || len < 1 || len > max_seq || kv_row_stride < (size_t)H * max_seq * 64)
            throw MaError(MA_ERR_INVALID, "ma_op_decode_attention_rows: bad arguments");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        if (halves == 2) {                                   // two blocks per (row, head): scratch granules + error word for this call
            unsigned long long* g = nullptr; unsigned* er = nullptr;
            HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&g), (size_t)B * H * ATTN_PAIR_GRANULES * sizeof(unsigned long long) + 64));
            er = reinterpret_cast<unsigned*>(g + (size_t)B * H * ATTN_PAIR_GRANULES);
            (void)hipMemsetAsync(g, 0, (size_t)B * H * ATTN_PAIR_GRANULES * sizeof(unsigned long long) + 64, s);
            hipError_t r = H16_CALL(g_op_hdt, HT, launch_attn_decode_final<HT>(q, kcache, vcache, H, max_seq, nullptr, len, 1, reinterpret_cast<bf16_t*>(out), H * 64, s, B, H * 64, kv_row_stride, 8, g, er, 3));
            unsigned herr = 0;
            (void)hipMemcpyAsync(&herr, er, sizeof(unsigned), hipMemcpyDeviceToHost, s);
            (void)hipStreamSynchronize(s);
            (void)hipFree(g);
            HIP_CHECK(r);
            if (herr) throw MaError(MA_ERR_HIP, "ma_op_decode_attention_rows: the hand-over between the two blocks of a pair timed out");
        } else if (halves == 1 || halves == 0) {
            HIP_CHECK(H16_CALL(g_op_hdt, HT, launch_attn_decode_final<HT>(q, kcache, vcache, H, max_seq, nullptr, len, 1, reinterpret_cast<bf16_t*>(out), H * 64, s, B, H * 64, kv_row_stride, waves)));
        } else throw MaError(MA_ERR_INVALID, "ma_op_decode_attention_rows: halves must be 1 or 2");
    });
}

// ---- batched decode step kernels (gemm_decode.hpp) --------------------------------------------------------------------
int ma_op_gemm_dec(const void* W, const float* bias, const void* xb, const float* res, float* y, void* yb, int N, int K, int B, int act, int ksplit,
                   void* stream) {
    return guarded(nullptr, [&] {
        if (!W || !xb || (!y && !yb)) throw MaError(MA_ERR_INVALID, "ma_op_gemm_dec: null pointer");
        GemmDecArgs a{};
        a.W = reinterpret_cast<const bf16_t*>(W); a.bias = bias; a.xb = reinterpret_cast<const bf16_t*>(xb); a.xb_stride = K;
        a.res = res; a.res_stride = N; a.y = y; a.y_stride = N; a.yb = reinterpret_cast<bf16_t*>(yb); a.yb_stride = N;
        a.N = N; a.K = K; a.B = B; a.act = act; a.epi = EPI_PLAIN; a.ksplit = ksplit;
        op_launched(H16_CALL(g_op_hdt, HT, launch_gemm_dec<HT>(a, reinterpret_cast<hipStream_t>(stream))), "ma_op_gemm_dec");
    });
}

int ma_op_gemm_dec_ln(const void* W, const float* bias, const float* pin, int parts, const float* pbias, const float* pres, const float* ln_g,
                      const float* ln_b, float eps, float* xn_out, float* y, void* yb, int N, int B, int act, void* stream) {
    return guarded(nullptr, [&] {
        if (!W || !pin || !ln_g || !ln_b || (!y && !yb)) throw MaError(MA_ERR_INVALID, "ma_op_gemm_dec_ln: null pointer");
        GemmDecArgs a{};
        a.W = reinterpret_cast<const bf16_t*>(W); a.bias = bias; a.y = y; a.y_stride = N; a.yb = reinterpret_cast<bf16_t*>(yb); a.yb_stride = N;
        a.N = N; a.K = 1024; a.B = B; a.act = act; a.epi = EPI_PLAIN; a.ksplit = 1;
        a.pin = pin; a.pin_stride = 1024; a.pin_parts = parts; a.pbias = pbias; a.pres = pres; a.pres_stride = 1024;
        a.ln_g = ln_g; a.ln_b = ln_b; a.ln_eps = eps; a.xn_out = xn_out; a.xn_stride = 1024;
        op_launched(H16_CALL(g_op_hdt, HT, launch_gemm_dec_ln<HT>(a, reinterpret_cast<hipStream_t>(stream))), "ma_op_gemm_dec_ln");
    });
}

int ma_op_gemm_dec_qkv(const void* W, const float* bias, const void* xb, float* q, void* kcache, void* vcache, int H, int max_seq, int pos, int B,
                       size_t kv_row_stride, void* stream) {
    return guarded(nullptr, [&] {
        if (!W || !xb || !q || !kcache || !vcache || pos < 0 || pos >= max_seq) throw MaError(MA_ERR_INVALID, "ma_op_gemm_dec_qkv: bad arguments");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        DecState* st = nullptr;
        HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&st), (size_t)B * sizeof(DecState)));
        try {
            HIP_CHECK(hipMemsetAsync(st, 0, (size_t)B * sizeof(DecState), s));
            hipLaunchKernelGGL(set_pos_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, s, st, 1, pos, 5, B);
            HIP_CHECK(hipGetLastError());
            GemmDecArgs a{};
            a.W = reinterpret_cast<const bf16_t*>(W); a.bias = bias; a.xb = reinterpret_cast<const bf16_t*>(xb); a.xb_stride = H;
            a.y = q; a.y_stride = H; a.N = 3 * H; a.K = H; a.B = B; a.ksplit = 1; a.epi = EPI_QKV;
            a.kcache = kcache; a.vcache = vcache; a.kv_row_stride = kv_row_stride; a.H = H; a.max_seq = max_seq; a.st = st;
            hipError_t r = H16_CALL(g_op_hdt, HT, launch_gemm_dec<HT>(a, s));
            if (r != hipSuccess) throw MaError(MA_ERR_HIP, std::string("ma_op_gemm_dec_qkv: ") + hipGetErrorString(r));
            HIP_CHECK(hipStreamSynchronize(s));
        } catch (...) { (void)hipFree(st); throw; }
        HIP_CHECK(hipFree(st));
    });
}

int ma_op_rows_prologue(int pro, const float* x, int nparts, int B, const float* bias, const float* res, const float* ln_g, const float* ln_b, float ln_eps,
                        const float* attn_ws, int attn_heads, float* xn_out, void* xb_out, int K, void* stream) {
    return guarded(nullptr, [&] {
        if (!xb_out || (pro != PRO_ATTN && !x) || (pro == PRO_ATTN && !attn_ws) || (pro == PRO_LN && (!ln_g || !ln_b)))
            throw MaError(MA_ERR_INVALID, "ma_op_rows_prologue: null pointer");
        RowsProArgs a{};
        a.x = x; a.x_stride = K; a.nparts = nparts < 1 ? 1 : nparts; a.B = B; a.bias = bias; a.res = res; a.res_stride = K;
        a.ln_g = ln_g; a.ln_b = ln_b; a.ln_eps = ln_eps; a.attn_ws = attn_ws; a.attn_ws_stride = attn_workspace_floats(attn_heads); a.attn_heads = attn_heads;
        a.xn_out = xn_out; a.xn_stride = K; a.xb = reinterpret_cast<bf16_t*>(xb_out); a.xb_stride = K; a.K = K;
        op_launched(H16_CALL(g_op_hdt, HT, launch_rows_prologue<HT>(a, pro, B, reinterpret_cast<hipStream_t>(stream))), "ma_op_rows_prologue");
    });
}

// the decode step's token pick on the caller's logits: pick_kernel<false> as enqueue_pick launches it (one block per row, V floats of dynamic LDS),
// on state records built here for step t
int ma_op_pick(const float* logits, int B, int V, const float* part_val, const int32_t* part_idx, int nparts, int do_sample, int top_k, float top_p,
               int suppress_eos, const float* uniforms, uint64_t seed, int t, int max_new, const int64_t* forced, int32_t* finished, int64_t* tokens,
               int32_t* cur_tok, void* stream) {
    return guarded(nullptr, [&] {
        if (!logits || !finished || !tokens || !cur_tok) throw MaError(MA_ERR_INVALID, "ma_op_pick: null pointer");
        if (B < 1 || B > 65535 || V < 3) throw MaError(MA_ERR_INVALID, "ma_op_pick: need 1 <= B <= 65535 and V >= 3");
        // (validate_config, engine_build.hpp: the V logits in dynamic LDS next to ~19 KB of static LDS, 64 KB per workgroup)
        if ((size_t)V * 4 + 20 * 1024 > 64 * 1024) throw MaError(MA_ERR_INVALID, "ma_op_pick: V too large for the sampler's LDS stage (max 11264)");
        if (nparts < 0 || nparts > V || (nparts > 0 && (!part_val || !part_idx))) throw MaError(MA_ERR_INVALID, "ma_op_pick: nparts must be in [0, V], with both partial arrays when > 0");
        if (t < 0 || max_new < 1) throw MaError(MA_ERR_INVALID, "ma_op_pick: need t >= 0 and max_new >= 1");
        if (do_sample && (top_k < 1 || top_k > PICK_KMAX)) throw MaError(MA_ERR_INVALID, "ma_op_pick: top_k must be in [1,64]");
        if (do_sample && !(top_p > 0.f && top_p <= 1.f)) throw MaError(MA_ERR_INVALID, "ma_op_pick: top_p must be in (0,1]");
        if (do_sample && uniforms && t >= max_new) throw MaError(MA_ERR_INVALID, "ma_op_pick: step t has no injected uniform (t >= max_new)");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        DecState* st = nullptr;
        HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&st), (size_t)B * sizeof(DecState)));
        try {
            DecState v{};
            v.suppress_eos = suppress_eos ? 1 : 0; v.do_sample = do_sample ? 1 : 0; v.top_k = top_k; v.top_p = top_p; v.seed = seed;
            v.uniforms = uniforms; v.max_new = max_new; v.forced = reinterpret_cast<const long long*>(forced);
            hipLaunchKernelGGL(init_state_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, s, st, v, B, V);
            HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(pick_state_in_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, s, st, t, finished, B);
            HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(pick_kernel<false>, dim3(B), dim3(256), (size_t)V * sizeof(float), s, logits, V, part_val, part_idx, nparts, nparts, st,
                               reinterpret_cast<long long*>(tokens), max_new, 0, PickEmbed{});
            HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(pick_state_out_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, s, st, finished, cur_tok, B);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipStreamSynchronize(s));
        } catch (...) { (void)hipFree(st); throw; }
        HIP_CHECK(hipFree(st));
    });
}

// the detokenizer's per-coordinate argmax (detok_chunk's last launch) on the caller's logits
int ma_op_coords_argmax(const float* logits, int nf, int nd, const uint8_t* mask, float* coords, void* stream) {
    return guarded(nullptr, [&] {
        if (!logits || !mask || !coords) throw MaError(MA_ERR_INVALID, "ma_op_coords_argmax: null pointer");
        if (nf < 1 || nf > (1 << 24) || nd < 1) throw MaError(MA_ERR_INVALID, "ma_op_coords_argmax: need 1 <= nf <= 2^24 and nd >= 1");
        hipLaunchKernelGGL(coords_argmax_kernel, dim3(ceil_div(nf * 9, 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), logits, nf, nd, mask, coords);
        HIP_CHECK(hipGetLastError());
    });
}

int ma_op_occupy_cus(int n_blocks, int lds_bytes, int64_t microseconds, const int32_t* release, void* stream) {
    return guarded(nullptr, [&] {
        if (n_blocks < 1 || n_blocks > 4096 || lds_bytes < 64 || lds_bytes > 160 * 1024 || microseconds < 1 || microseconds > 2000000)
            throw MaError(MA_ERR_INVALID, "ma_op_occupy_cus: bad arguments");
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(occupy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
        hipLaunchKernelGGL(occupy_kernel, dim3(n_blocks), dim3(64), (size_t)lds_bytes, reinterpret_cast<hipStream_t>(stream), (unsigned long long)microseconds * 100ull,
                           reinterpret_cast<const int*>(release), (unsigned*)nullptr);
        HIP_CHECK(hipGetLastError());
    });
}

int ma_op_set_half_dtype(int dtype) {
    if (dtype != MA_DTYPE_BF16 && dtype != MA_DTYPE_F16) return MA_ERR_INVALID;
    g_op_hdt = dtype;
    return MA_OK;
}

int ma_op_stream_copy(void* dst, const void* src, size_t bytes, int mode, void* stream) {
    return guarded(nullptr, [&] {
        if (!dst || !src || bytes % 16 || mode < 0 || mode > 2) throw MaError(MA_ERR_INVALID, "ma_op_stream_copy: null pointer, size not a multiple of 16 or mode outside 0 .. 2");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        const size_t n16 = bytes / 16;
        const u32x4* sp = reinterpret_cast<const u32x4*>(src); u32x4* dp = reinterpret_cast<u32x4*>(dst);
        if (mode == 0) hipLaunchKernelGGL(stream_copy_kernel<0>, dim3(2048), dim3(256), 0, s, sp, dp, n16);
        else if (mode == 1) hipLaunchKernelGGL(stream_copy_kernel<1>, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, s, sp, dp, n16);
        else hipLaunchKernelGGL(stream_copy_kernel<2>, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, s, sp, dp, n16);
        HIP_CHECK(hipGetLastError());
    });
}

size_t ma_decode_attention_workspace_bytes(int H) {
    if (H < 1) return 0;
    return attn_workspace_floats(H) * sizeof(float);
}

// ---- measurement ---------------------------------------------------------------------------------------------------
int ma_profile_decode(ma_engine* e, int kv_len, int steps, ma_kernel_timing* out, void* stream) {
    if (!e || !out) return MA_ERR_INVALID;
    return guarded(e, [&] {
        require_ready(e);
        if (steps < 1 || steps > 64) throw MaError(MA_ERR_INVALID, "steps must be in [1,64]");
        if (kv_len < e->T + 1 || kv_len + 3 * steps + 8 > e->maxseq) throw MaError(MA_ERR_INVALID, "kv_len out of range");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        std::memset(out, 0, sizeof(*out));
        const int B = std::max(1, std::min(e->opt.profile_batch, e->cfg.max_batch));
        const int impl = persist_selected(e, B, 0) ? 1 : 0;
        if (impl == 1 || embed_from_table(e, B)) ensure_embtab(e, s);
        ensure_graphs(e, B, impl);
        auto reset = [&] { state_at(e, s, B, kv_len); };
        hipEvent_t a, b;
        HIP_CHECK(hipEventCreate(&a)); HIP_CHECK(hipEventCreate(&b));
        // One event pair around `steps` back-to-back steps (no per-launch events: an event record between two launches
        // costs more than the launch boundary it would measure).  only_cls >= 0 enqueues just that class of launches, so
        // class time / launches is the average launch duration, boundary to the next launch included -- the same view as
        // a rocprofv3 kernel trace of the replayed graph.  only_cls == -2: graph replays (with row groups on their streams when
        // decode_groups > 1; the per-class and eager figures are always one ungrouped chain on `s`).
        auto timed = [&](int only_cls, int* launches) -> float {
            StepTimer tm; tm.only_cls = only_cls;
            Step step(e, s, tm, Rows{0, B});
            reset();
            if (only_cls == -2) launch_steps(e, s, B, impl, 1);                                   // warm
            else { StepTimer w; w.only_cls = only_cls; Step warm(e, s, w, Rows{0, B}); enqueue_decode_step(warm, impl); }
            reset();
            HIP_CHECK(hipEventRecord(a, s));
            if (only_cls == -2) launch_steps(e, s, B, impl, steps);          // what generate() runs: row groups on their streams, joined on s
            else for (int i = 0; i < steps; ++i) {
                enqueue_decode_step(step, impl);
                if (only_cls >= 0 && only_cls != CLS_PICK) {
                    // without the pick launch the state would not advance, and the fused launches tag their in-launch exchanges
                    // with the cache position: move it by hand (one tiny launch per step, charged to the class being timed)
                    hipLaunchKernelGGL(set_pos_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, s, e->d_st, kv_len - e->T + i + 1, kv_len + i, 5, B);
                    HIP_CHECK(hipGetLastError());
                }
            }
            HIP_CHECK(hipEventRecord(b, s));
            HIP_CHECK(hipStreamSynchronize(s));
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, a, b));
            if (launches) *launches = only_cls >= 0 ? tm.launched[only_cls] : 0;
            return ms;
        };
        out->step_ms_eager = timed(-1, nullptr) / steps;
        if (e->cfg.use_graph) out->step_ms_graph = timed(-2, nullptr) / steps;
        for (LaunchClass cls : {CLS_WEIGHTS, CLS_ATTN, CLS_PERSIST, CLS_PICK}) {
            if ((impl == 1) != (cls == CLS_PERSIST)) continue;          // the persistent step is one launch of its own class
            int n = 0;
            out->ms[cls] = timed(cls, &n);
            out->launches[cls] = n;
        }
        (void)hipEventDestroy(a); (void)hipEventDestroy(b);
        if (impl == 1) check_persist_error(e, s);
        else check_chain_error(e, s);                       // timings of zero-filled exchanges are not timings
    });
}

int ma_trace_decode(ma_engine* e, int kv_len, uint64_t* host_out, int max_launches, int max_blocks, int32_t* kinds, int32_t* blocks, int32_t* n_launches,
                    void* stream) {
    if (!e || !host_out || !kinds || !blocks || !n_launches || max_launches < 1 || max_blocks < 1) return MA_ERR_INVALID;
    return guarded(e, [&] {
        require_ready(e);
        if (kv_len < e->T + 1 || kv_len + 16 > e->maxseq) throw MaError(MA_ERR_INVALID, "kv_len out of range");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        const int TB = std::max(1, std::min(e->opt.profile_batch, e->cfg.max_batch));      // rows of the traced step (option profile_batch)
        if (embed_from_table(e, TB)) ensure_embtab(e, s);
        state_at(e, s, TB, kv_len);      // (embed_table: includes the one embedding launch that feeds the first step; trace kind 0 then has no slot)
        const size_t n64 = (size_t)max_launches * max_blocks * 4;
        unsigned long long* d_tr = nullptr;
        HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_tr), n64 * sizeof(unsigned long long)));
        try {
            HIP_CHECK(hipMemsetAsync(d_tr, 0, n64 * sizeof(unsigned long long), s));
            StepTimer none;
            Step warm(e, s, none, Rows{0, TB});
            for (int i = 0; i < 3; ++i) enqueue_decode_step(warm);            // warm: clocks, caches
            std::vector<int> k, b;                                            // TraceKind per traced launch, its blocks
            StepTimer tm; tm.tr = d_tr; tm.tr_max_launches = max_launches; tm.tr_max_blocks = max_blocks; tm.tr_kind = &k; tm.tr_blocks = &b;
            Step traced(e, s, tm, Rows{0, TB});
            enqueue_decode_step(traced);
            HIP_CHECK(hipMemcpyAsync(host_out, d_tr, n64 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            *n_launches = (int)k.size();
            for (size_t i = 0; i < k.size(); ++i) { kinds[i] = k[i]; blocks[i] = b[i]; }
            check_chain_error(e, s);
        } catch (...) { (void)hipFree(d_tr); throw; }
        HIP_CHECK(hipFree(d_tr));
    });
}

// In-kernel timeline of ONE persistent decode step (diagnostics; MA_EXPERIMENTAL libraries): for every workgroup, the 100 MHz real-time counter at kernel
// start, then two stamps per edge (local share published = start of the sweep | gather complete), then the end.
int ma_persist_trace(ma_engine* e, int kv_len, uint64_t* host_out, int32_t* n_events, void* stream) {
    if (!e || !host_out || !n_events) return MA_ERR_INVALID;
    return guarded(e, [&] { persist_trace(e, kv_len, host_out, n_events, reinterpret_cast<hipStream_t>(stream)); });
}

// the last decode step's logits of batch row `row` (V floats, device -> caller's device buffer): parity tests compare the two
// step implementations bit for bit
int ma_engine_read_logits(ma_engine* e, int row, float* out, void* stream) {
    if (!e || !out) return MA_ERR_INVALID;
    return guarded(e, [&] {
        if (row < 0 || row >= e->cfg.max_batch) throw MaError(MA_ERR_INVALID, "row out of range");
        HIP_CHECK(hipMemcpyAsync(out, e->d_logits + (size_t)row * e->V, (size_t)e->V * sizeof(float), hipMemcpyDeviceToDevice, reinterpret_cast<hipStream_t>(stream)));
    });
}

// test aid (tests/test_gpu_embed_table.py): `n` rows of hidden floats into the caller's device buffer.
// what 0: rows [row0, row0 + n) of the embedding table (built first when the weights changed since).
// what 1: what the step's embedding launch (gemv_kernel, EPI_EMBED) computes for the tokens row0 + 3 .. row0 + n + 2 in front of its positional adds: the
//         launch itself, one token at a time through batch row 0's state record, with all-zero tables in place of the three positional ones.
int ma_engine_embed_rows(ma_engine* e, int what, int row0, int n, float* out, void* stream) {
    if (!e || !out) return MA_ERR_INVALID;
    return guarded(e, [&] {
        require_ready(e);
        const ma_config& c = e->cfg;
        if ((what != 0 && what != 1) || row0 < 0 || n < 1 || row0 > c.codebook_size - n) throw MaError(MA_ERR_INVALID, "ma_engine_embed_rows: what must be 0 or 1, the rows inside [0, codebook_size)");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        const size_t H = c.hidden;
        if (what == 0) {
            ensure_embtab(e, s);
            HIP_CHECK(hipMemcpyAsync(out, e->d_embtab + (size_t)row0 * H, (size_t)n * H * sizeof(float), hipMemcpyDeviceToDevice, s));
            return;
        }
        // step 0 reads slot row 10 of token_embed_positions, row 1 of cond_embed and row T + 1 of embed_positions
        const size_t zrows = (size_t)std::max(e->T + 2, 12);
        float* z = nullptr;
        HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&z), zrows * H * sizeof(float)));
        try {
            HIP_CHECK(hipMemsetAsync(z, 0, zrows * H * sizeof(float), s));
            StepTimer none;
            const Step row0_step(e, s, none, Rows{0, 1});
            for (int i = 0; i < n; ++i) {
                hipLaunchKernelGGL(set_pos_kernel, dim3(1), dim3(64), 0, s, e->d_st, 0, e->T - 1, row0 + i + 3, 1);
                HIP_CHECK(hipGetLastError());
                GemvArgs a = make_embed_args(row0_step);
                a.tokpos = z; a.cond = z; a.postab = z; a.y = out + (size_t)i * H;
                gemv_launch(e, a, s, 1);
            }
            HIP_CHECK(hipStreamSynchronize(s));
        } catch (...) { (void)hipFree(z); throw; }
        HIP_CHECK(hipFree(z));
    });
}

// 1 when the persistent decode step can run on this engine (bf16, 350M layer shape, 256-CU device), else 0
int ma_engine_persist_available(ma_engine* e) { return e && e->persist_shape ? 1 : 0; }

// ---- watertight remeshing (csrc/watertight.hpp) -----------------------------------------------------------------------------
size_t ma_mesh_udf_workspace_bytes(int nf) { return nf < 1 || nf > MA_MESH_UDF_MAX_FACES ? 0 : wt::udf_ws_bytes(nf); }

int ma_op_mesh_udf(const float* verts, int nv, const int32_t* faces, int nf, int size, float* field, void* workspace, size_t ws_bytes, void* stream) {
    return guarded(nullptr, [&] {
        if (!verts || !faces || !field || !workspace) throw MaError(MA_ERR_INVALID, "ma_op_mesh_udf: null pointer");
        if (nv < 1 || nf < 1 || nf > MA_MESH_UDF_MAX_FACES || size < 2 || size > 512)
            throw MaError(MA_ERR_INVALID, "ma_op_mesh_udf: need nv >= 1, 1 <= nf <= 2^28 and size in [2, 512]");
        if (ws_bytes < wt::udf_ws_bytes(nf)) throw MaError(MA_ERR_INVALID, "ma_op_mesh_udf: workspace smaller than ma_mesh_udf_workspace_bytes(nf)");
        HIP_CHECK(wt::launch_mesh_udf(verts, nv, faces, nf, size, field, workspace, reinterpret_cast<hipStream_t>(stream)));
    });
}

size_t ma_marching_cubes_workspace_bytes(int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2) return 0;
    return wt::mc_ws_bytes((int64_t)nx * ny * nz);
}

int ma_op_marching_cubes(const float* field, int nx, int ny, int nz, float level, float* verts, int64_t max_verts, int32_t* tris, int64_t max_tris,
                         int64_t* counts, void* workspace, size_t ws_bytes, void* stream) {
    return guarded(nullptr, [&] {
        if (!field || !counts || !workspace) throw MaError(MA_ERR_INVALID, "ma_op_marching_cubes: null field, counts or workspace");
        if (nx < 2 || ny < 2 || nz < 2 || (int64_t)nx * ny * nz > (int64_t(1) << 30))
            throw MaError(MA_ERR_INVALID, "ma_op_marching_cubes: need nx, ny, nz >= 2 and at most 2^30 grid points");
        if (!std::isfinite(level)) throw MaError(MA_ERR_INVALID, "ma_op_marching_cubes: non-finite level");
        if ((verts == nullptr) != (tris == nullptr)) throw MaError(MA_ERR_INVALID, "ma_op_marching_cubes: verts and tris must both be given or both be NULL");
        const int64_t np = (int64_t)nx * ny * nz;
        if (ws_bytes < wt::mc_ws_bytes(np)) throw MaError(MA_ERR_INVALID, "ma_op_marching_cubes: workspace smaller than ma_marching_cubes_workspace_bytes(nx, ny, nz)");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        wt::McWs ws;
        wt::mc_ws_bytes(np, &ws, workspace);
        HIP_CHECK(wt::launch_mc_count(field, nx, ny, nz, level, ws, s));
        int64_t tot[2];
        HIP_CHECK(hipMemcpyAsync(&tot[0], ws.vcount + np, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(&tot[1], ws.tcount + np, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        counts[0] = tot[0];
        counts[1] = tot[1];
        if (tot[0] > INT32_MAX) throw MaError(MA_ERR_INVALID, "ma_op_marching_cubes: more than 2^31 - 1 vertices");
        if (!verts) return;
        if (tot[0] > max_verts || tot[1] > max_tris)
            throw MaError(MA_ERR_CAPACITY, "ma_op_marching_cubes: " + std::to_string(tot[0]) + " vertices / " + std::to_string(tot[1]) +
                                               " triangles do not fit in max_verts " + std::to_string(max_verts) + " / max_tris " + std::to_string(max_tris));
        HIP_CHECK(wt::launch_mc_emit(field, nx, ny, nz, level, ws, verts, max_verts, tris, max_tris, s));
    });
}

int ma_mc_table(int8_t* tris, int8_t* edges, int32_t* max_tris_per_cell) {
    if (max_tris_per_cell) *max_tris_per_cell = wt::MC_MAX_TRIS;
    if (tris) std::memcpy(tris, wt::MC_TRIS_HOST, sizeof(wt::MC_TRIS_HOST));
    if (edges) std::memcpy(edges, wt::MC_EDGES_HOST, sizeof(wt::MC_EDGES_HOST));
    return MA_OK;
}


// ---- surface sampling (csrc/surface_sample.hpp) -----------------------------------------------------------------------------
size_t ma_surface_sample_workspace_bytes(int nf) { return nf < 1 || nf > MA_SURFACE_SAMPLE_MAX_FACES ? 0 : ss::cdf_ws_bytes(nf); }

int ma_op_mc_vertices_to_frame(const float* index_verts, int nv, int size, double to_orig_scale, const double* center, double* verts, void* stream) {
    return guarded(nullptr, [&] {
        if (!index_verts || !center || !verts) throw MaError(MA_ERR_INVALID, "ma_op_mc_vertices_to_frame: null pointer");
        if (nv < 1 || size < 1) throw MaError(MA_ERR_INVALID, "ma_op_mc_vertices_to_frame: need nv >= 1 and size >= 1");
        if (!std::isfinite(to_orig_scale) || !(to_orig_scale != 0.0)) throw MaError(MA_ERR_INVALID, "ma_op_mc_vertices_to_frame: to_orig_scale must be finite and non-zero");
        HIP_CHECK(ss::launch_frame(index_verts, nv, size, to_orig_scale, center, verts, reinterpret_cast<hipStream_t>(stream)));
    });
}

int ma_op_surface_cdf(const double* verts, int nv, const int32_t* faces, int nf, double* normals, double* cum, void* workspace, size_t ws_bytes,
                      void* stream) {
    return guarded(nullptr, [&] {
        if (!verts || !faces || !normals || !cum || !workspace) throw MaError(MA_ERR_INVALID, "ma_op_surface_cdf: null pointer");
        if (nv < 1 || nf < 1 || nf > MA_SURFACE_SAMPLE_MAX_FACES) throw MaError(MA_ERR_INVALID, "ma_op_surface_cdf: need nv >= 1 and 1 <= nf <= 2^28");
        if (ws_bytes < ss::cdf_ws_bytes(nf)) throw MaError(MA_ERR_INVALID, "ma_op_surface_cdf: workspace smaller than ma_surface_sample_workspace_bytes(nf)");
        HIP_CHECK(ss::launch_surface_cdf(verts, nv, faces, nf, normals, cum, workspace, reinterpret_cast<hipStream_t>(stream)));
    });
}

int ma_op_sample_surface(const double* verts, int nv, const int32_t* faces, int nf, const double* normals, const double* cum, const double* u,
                         const double* uv, int count, uint16_t* out, int64_t* face_idx, void* stream) {
    return guarded(nullptr, [&] {
        if (!verts || !faces || !normals || !cum || !u || !uv || !out) throw MaError(MA_ERR_INVALID, "ma_op_sample_surface: null pointer");
        if (nv < 1 || nf < 1 || nf > MA_SURFACE_SAMPLE_MAX_FACES || count < 1)
            throw MaError(MA_ERR_INVALID, "ma_op_sample_surface: need nv >= 1, 1 <= nf <= 2^28 and count >= 1");
        HIP_CHECK(ss::launch_draw(verts, nv, faces, nf, normals, cum, u, uv, count, out, face_idx, reinterpret_cast<hipStream_t>(stream)));
    });
}

int ma_f64_to_f16(const double* x, int64_t n, uint16_t* out) {
    if (!x || !out || n < 0) return MA_ERR_INVALID;
    for (int64_t i = 0; i < n; ++i) out[i] = ss::f64_to_f16_rne(x[i]);
    return MA_OK;
}

// ---- best-of-N candidate scores (csrc/mesh_score.hpp) -------------------------------------------------------------------------
static bool score_shape_ok(int B, int F, int P) { return B >= 1 && F >= 1 && F <= MA_SCORE_MESHES_MAX_FACES && P >= 1 && P <= MA_SCORE_MESHES_MAX_POINTS; }

size_t ma_score_meshes_workspace_bytes(int B, int F, int P) { return score_shape_ok(B, F, P) ? score::score_ws_bytes(B, F, P) : 0; }

int ma_op_score_meshes(const float* coords, int B, int F, const float* cloud, int cloud_ld, int P, int n_per_cloud, float mesh_scale, float* scores,
                       void* workspace, size_t ws_bytes, void* stream) {
    return guarded(nullptr, [&] {
        if (!coords || !cloud || !scores || !workspace) throw MaError(MA_ERR_INVALID, "ma_op_score_meshes: null pointer");
        if (!score_shape_ok(B, F, P)) throw MaError(MA_ERR_INVALID, "ma_op_score_meshes: need B >= 1, 1 <= F <= 2^20 and 1 <= P <= 2^20");
        if (n_per_cloud < 1 || B % n_per_cloud) throw MaError(MA_ERR_INVALID, "ma_op_score_meshes: n_per_cloud must be >= 1 and divide B");
        if (cloud_ld != 3 && cloud_ld != 6) throw MaError(MA_ERR_INVALID, "ma_op_score_meshes: cloud_ld must be 3 or 6");
        if (!std::isfinite(mesh_scale) || !(mesh_scale > 0.f)) throw MaError(MA_ERR_INVALID, "ma_op_score_meshes: mesh_scale must be finite and > 0");
        if (ws_bytes < score::score_ws_bytes(B, F, P)) throw MaError(MA_ERR_INVALID, "ma_op_score_meshes: workspace smaller than ma_score_meshes_workspace_bytes(B, F, P)");
        HIP_CHECK(score::launch_score_meshes(coords, B, F, cloud, cloud_ld, P, n_per_cloud, mesh_scale, scores, workspace, reinterpret_cast<hipStream_t>(stream)));
    });
}

// ---- normal agreement of candidate meshes with their cloud (csrc/mesh_normals.hpp) --------------------------------------------
static bool mesh_normals_shape_ok(int B, int F) { return B >= 1 && F >= 1 && F <= MA_SCORE_MESHES_MAX_FACES; }

size_t ma_mesh_normals_workspace_bytes(int B, int F) { return mesh_normals_shape_ok(B, F) ? mnorm::normals_ws_bytes(B, F) : 0; }

int ma_op_mesh_normals(const float* coords, int B, int F, const float* cloud, int cloud_ld, int P, int n_per_cloud, float mesh_scale, float* face_agree,
                       float* nscores, void* workspace, size_t ws_bytes, void* stream) {
    return guarded(nullptr, [&] {
        if (!coords || !cloud || !face_agree || !nscores || !workspace) throw MaError(MA_ERR_INVALID, "ma_op_mesh_normals: null pointer");
        if (!score_shape_ok(B, F, P)) throw MaError(MA_ERR_INVALID, "ma_op_mesh_normals: need B >= 1, 1 <= F <= 2^20 and 1 <= P <= 2^20");
        if (n_per_cloud < 1 || B % n_per_cloud) throw MaError(MA_ERR_INVALID, "ma_op_mesh_normals: n_per_cloud must be >= 1 and divide B");
        if (cloud_ld != 6) throw MaError(MA_ERR_INVALID, "ma_op_mesh_normals: cloud_ld must be 6 (xyz and the normal)");
        if (!std::isfinite(mesh_scale) || !(mesh_scale > 0.f)) throw MaError(MA_ERR_INVALID, "ma_op_mesh_normals: mesh_scale must be finite and > 0");
        if (ws_bytes < mnorm::normals_ws_bytes(B, F)) throw MaError(MA_ERR_INVALID, "ma_op_mesh_normals: workspace smaller than ma_mesh_normals_workspace_bytes(B, F)");
        HIP_CHECK(mnorm::launch_mesh_normals(coords, B, F, cloud, cloud_ld, P, n_per_cloud, mesh_scale, face_agree, nscores, workspace,
                                             reinterpret_cast<hipStream_t>(stream)));
    });
}

// ---- fit of a generated mesh to its cloud: pairing and per-face sums (csrc/mesh_fit.hpp) ----------------------------------------
static bool mesh_fit_shape_ok(int V, int M, int P) {
    return M >= 1 && M <= MA_MESH_FIT_MAX_FACES && V >= 1 && V <= 3 * M && P >= 1 && P <= MA_MESH_FIT_MAX_POINTS;
}

size_t ma_mesh_fit_workspace_bytes(int V, int M, int P) { return mesh_fit_shape_ok(V, M, P) ? fit::fit_ws_bytes(P) : 0; }

int ma_op_mesh_fit_pairs(const float* verts, int V, const int32_t* faces, int M, const float* cloud, int cloud_ld, int P, float dist, float min_cos, float flat,
                         int32_t* pt_face, float* pt_w, int64_t* face_sums, void* workspace, size_t ws_bytes, void* stream) {
    return guarded(nullptr, [&] {
        if (!mesh_fit_shape_ok(V, M, P)) throw MaError(MA_ERR_INVALID, "ma_op_mesh_fit_pairs: need 1 <= M <= 4096, 1 <= V <= 3 M and 1 <= P <= 2^22");
        if (!verts || !faces || !cloud || !pt_face || !pt_w || !face_sums || !workspace) throw MaError(MA_ERR_INVALID, "ma_op_mesh_fit_pairs: null pointer");
        if (cloud_ld != 6) throw MaError(MA_ERR_INVALID, "ma_op_mesh_fit_pairs: cloud_ld must be 6 (xyz and the normal)");
        if (!std::isfinite(dist) || !(dist > 0.f) || dist > 1.0f) throw MaError(MA_ERR_INVALID, "ma_op_mesh_fit_pairs: dist must be finite, > 0 and at most 1");
        if (!(min_cos >= 0.f && min_cos < 1.0f)) throw MaError(MA_ERR_INVALID, "ma_op_mesh_fit_pairs: min_cos must be in [0, 1)");
        if (!std::isfinite(flat) || !(flat >= 0.f)) throw MaError(MA_ERR_INVALID, "ma_op_mesh_fit_pairs: flat must be finite and >= 0");
        if (ws_bytes < fit::fit_ws_bytes(P)) throw MaError(MA_ERR_INVALID, "ma_op_mesh_fit_pairs: workspace smaller than ma_mesh_fit_workspace_bytes(V, M, P)");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        HIP_CHECK(fit::launch_mesh_fit_pairs(verts, V, faces, M, cloud, cloud_ld, P, dist, min_cos, flat, pt_face, pt_w, face_sums, workspace, s));
        fit::FitWs ws;
        fit::fit_ws_bytes(P, &ws, workspace);
        int status = 0;                                              // what the kernels found in the arrays themselves
        HIP_CHECK(hipMemcpyAsync(&status, ws.status, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (status & fit::ST_FACE_INDEX) throw MaError(MA_ERR_INVALID, "ma_op_mesh_fit_pairs: a face index is outside 0 .. V - 1");
        if (status & fit::ST_VERT_NONFINITE) throw MaError(MA_ERR_INVALID, "ma_op_mesh_fit_pairs: a vertex of a face has a non-finite coordinate");
        if (status & fit::ST_CLOUD_NONFINITE) throw MaError(MA_ERR_INVALID, "ma_op_mesh_fit_pairs: the cloud has a non-finite coordinate or normal");
    });
}

// ---- normals of a raw point cloud (csrc/pc_normals.hpp) -----------------------------------------------------------------------
static bool pc_knn_shape_ok(int N, int Q, int k, int splits) {
    return k >= MA_PC_KNN_MIN_K && k <= MA_PC_KNN_MAX_K && N >= k && N <= MA_PC_KNN_MAX_POINTS && Q >= 1 && Q <= MA_PC_KNN_MAX_QUERIES && splits >= 0 &&
           splits <= MA_PC_KNN_MAX_SPLITS;
}

size_t ma_pc_knn_workspace_bytes(int N, int Q, int k, int splits) { return pc_knn_shape_ok(N, Q, k, splits) ? pcn::knn_ws_bytes(N, Q, k, splits) : 0; }

int ma_op_pc_knn(const float* ref, int N, int ref_ld, const int32_t* query_idx, int Q, int k, int splits, int32_t* nbr_idx, float* nbr_d2, void* workspace,
                 size_t ws_bytes, void* stream) {
    return guarded(nullptr, [&] {
        if (!ref || !nbr_idx || !nbr_d2 || !workspace) throw MaError(MA_ERR_INVALID, "ma_op_pc_knn: null pointer");
        if (!pc_knn_shape_ok(N, Q, k, splits))
            throw MaError(MA_ERR_INVALID, "ma_op_pc_knn: need 3 <= k <= 32, k <= N <= 2^22, 1 <= Q <= 2^20 and 0 <= splits <= 64");
        if (ref_ld != 3 && ref_ld != 6) throw MaError(MA_ERR_INVALID, "ma_op_pc_knn: ref_ld must be 3 or 6");
        if (!query_idx && Q != N) throw MaError(MA_ERR_INVALID, "ma_op_pc_knn: without query_idx every reference point is a query: Q must equal N");
        if (ws_bytes < pcn::knn_ws_bytes(N, Q, k, splits)) throw MaError(MA_ERR_INVALID, "ma_op_pc_knn: workspace smaller than ma_pc_knn_workspace_bytes(N, Q, k, splits)");
        HIP_CHECK(pcn::launch_knn(ref, N, ref_ld, query_idx, Q, k, pcn::resolve_splits(N, Q, splits), nbr_idx, nbr_d2, workspace,
                                  reinterpret_cast<hipStream_t>(stream)));
    });
}

int ma_op_pc_normals(const float* ref, int N, int ref_ld, const int32_t* nbr_idx, int Q, int k, double* normals, double* eigvals, void* stream) {
    return guarded(nullptr, [&] {
        if (!ref || !nbr_idx || !normals || !eigvals) throw MaError(MA_ERR_INVALID, "ma_op_pc_normals: null pointer");
        if (!pc_knn_shape_ok(N, Q, k, 0)) throw MaError(MA_ERR_INVALID, "ma_op_pc_normals: need 3 <= k <= 32, k <= N <= 2^22 and 1 <= Q <= 2^20");
        if (ref_ld != 3 && ref_ld != 6) throw MaError(MA_ERR_INVALID, "ma_op_pc_normals: ref_ld must be 3 or 6");
        HIP_CHECK(pcn::launch_normals(ref, N, ref_ld, nbr_idx, Q, k, normals, eigvals, reinterpret_cast<hipStream_t>(stream)));
    });
}

// ---- farthest-point sampling of a point cloud (csrc/pc_fps.hpp) ------------------------------------------------------------------
static_assert(MA_PC_FPS_MAX_POINTS == fps::MAX_POINTS && MA_PC_FPS_ONE_MAX_POINTS == fps::ONE_MAX_POINTS, "the header's limits are the kernels'");
static bool pc_fps_shape_ok(int N, int n, int form) {
    return n >= 1 && n <= N && N <= MA_PC_FPS_MAX_POINTS && n <= MA_PC_FPS_MAX_PICKS && form >= 0 && form <= 2;
}

size_t ma_pc_fps_workspace_bytes(int N, int n, int form) { return pc_fps_shape_ok(N, n, form) ? fps::layout(N).bytes : 0; }

int ma_op_pc_fps(const float* ref, int N, int ref_ld, int n, int start, int form, int32_t* idx, float* d2, void* workspace, size_t ws_bytes, void* stream) {
    return guarded(nullptr, [&] {
        if (!ref || !idx || !d2 || !workspace) throw MaError(MA_ERR_INVALID, "ma_op_pc_fps: null pointer");
        if (!pc_fps_shape_ok(N, n, form)) throw MaError(MA_ERR_INVALID, "ma_op_pc_fps: need 1 <= n <= N <= 2^22, n <= 2^16 and form in 0..2");
        if (ref_ld != 3 && ref_ld != 6) throw MaError(MA_ERR_INVALID, "ma_op_pc_fps: ref_ld must be 3 or 6");
        if (start < -1 || start >= N) throw MaError(MA_ERR_INVALID, "ma_op_pc_fps: start must be -1 or a row in [0, N)");
        if (form == 1 && N > fps::ONE_MAX_POINTS)
            throw MaError(MA_ERR_INVALID, "ma_op_pc_fps: form 1 (one workgroup) holds at most MA_PC_FPS_ONE_MAX_POINTS = 16384 points");
        if (ws_bytes < fps::layout(N).bytes) throw MaError(MA_ERR_INVALID, "ma_op_pc_fps: workspace smaller than ma_pc_fps_workspace_bytes(N, n, form)");
        HIP_CHECK(fps::launch_fps(ref, N, ref_ld, n, start, fps::resolve_form(N, form), idx, d2, workspace, reinterpret_cast<hipStream_t>(stream)));
    });
}

// ---- neighbours of every point over a cell grid, for statistical outlier removal (csrc/pc_grid.hpp) -------------------------------------
static_assert(MA_PC_GRID_MAX_POINTS == pcg::MAX_POINTS && MA_PC_GRID_MAX_DIM == pcg::MAX_DIM && MA_PC_GRID_MAX_CELLS == pcg::MAX_CELLS,
              "the header's limits are the kernels'");
static bool grid_dims_ok(int nx, int ny, int nz) {
    return nx >= 1 && nx <= MA_PC_GRID_MAX_DIM && ny >= 1 && ny <= MA_PC_GRID_MAX_DIM && nz >= 1 && nz <= MA_PC_GRID_MAX_DIM &&
           (int64_t)nx * ny * nz <= MA_PC_GRID_MAX_CELLS;
}

static bool pc_grid_n_ok(int N, int k) { return k >= MA_PC_KNN_MIN_K && k <= MA_PC_KNN_MAX_K && N >= k && N <= MA_PC_GRID_MAX_POINTS; }

// the grid of a grid op, checked; n_ok / need: the op's own test of N (and k) and its wording
static pcg::Grid checked_grid(const std::string& op, bool n_ok, const char* need, const float* origin, float cell, const int32_t* dims) {
    if (!n_ok || !grid_dims_ok(dims[0], dims[1], dims[2])) throw MaError(MA_ERR_INVALID, op + ": need " + need + ", every dim in 1..128 and at most 2^21 cells");
    if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2])) throw MaError(MA_ERR_INVALID, op + ": origin must be finite");
    if (!std::isfinite(cell) || !(cell > 0.f)) throw MaError(MA_ERR_INVALID, op + ": cell must be finite and > 0");
    return pcg::Grid{origin[0], origin[1], origin[2], cell, dims[0], dims[1], dims[2]};
}

size_t ma_pc_knn_grid_workspace_bytes(int N, int k, int nx, int ny, int nz) { return pc_grid_n_ok(N, k) && grid_dims_ok(nx, ny, nz) ? pcg::layout(N, nx * ny * nz).bytes : 0; }

int ma_op_pc_knn_grid(const float* ref, int N, int ref_ld, int k, const float* origin, float cell, const int32_t* dims, int32_t* nbr_idx, float* nbr_d2,
                      double* mean_dist, void* workspace, size_t ws_bytes, void* stream) {
    return guarded(nullptr, [&] {
        if (!ref || !origin || !dims || !workspace) throw MaError(MA_ERR_INVALID, "ma_op_pc_knn_grid: null pointer");
        if (!nbr_idx && !nbr_d2 && !mean_dist) throw MaError(MA_ERR_INVALID, "ma_op_pc_knn_grid: no output: give at least one of nbr_idx, nbr_d2 and mean_dist");
        const pcg::Grid g = checked_grid("ma_op_pc_knn_grid", pc_grid_n_ok(N, k), "3 <= k <= 32, k <= N <= 2^22", origin, cell, dims);
        if (ref_ld != 3 && ref_ld != 6) throw MaError(MA_ERR_INVALID, "ma_op_pc_knn_grid: ref_ld must be 3 or 6");
        if (ws_bytes < pcg::layout(N, pcg::cells_of(g)).bytes)
            throw MaError(MA_ERR_INVALID, "ma_op_pc_knn_grid: workspace smaller than ma_pc_knn_grid_workspace_bytes(N, k, nx, ny, nz)");
        HIP_CHECK(pcg::launch_build(ref, N, ref_ld, g, workspace, reinterpret_cast<hipStream_t>(stream)));
        HIP_CHECK(pcg::launch_search(N, k, g, nbr_idx, nbr_d2, mean_dist, workspace, reinterpret_cast<hipStream_t>(stream)));
    });
}

// ---- the radius searches over the cell grid: what cluster, smooth and upsample share on the host (csrc/pc_radius.hpp) ------------------------
static bool pc_radius_shape_ok(int N, int nx, int ny, int nz) { return N >= 1 && N <= MA_PC_GRID_MAX_POINTS && grid_dims_ok(nx, ny, nz); }

// called before the op's own checks, so that an N outside the limits is reported as that and not by a check that multiplies by it
static pcg::Grid radius_grid(const std::string& op, int N, const float* origin, float cell, const int32_t* dims) {
    return checked_grid(op, N >= 1 && N <= MA_PC_GRID_MAX_POINTS, "1 <= N <= 2^22", origin, cell, dims);
}

// From the checked grid and the op's own checked arguments to the point where the op's long kernel may be launched: the ratio rule (`what`
// names the radius in it), r2 = fl32(radius * radius) with radius as float32, the rings and the host's test that they suffice, the workspace
// size (need_bytes: the op's layout), the build and the pair bound, its read-back into *pair_bound, and the cap.  Returns r2.  zeroed, if
// given: a result of the op that is 0 from the moment the checks have passed (upsample's total).
static float radius_prologue(const std::string& name, const char* what, const float* ref, int N, int ref_ld, const pcg::Grid& g, double radius,
                             uint64_t max_pairs, void* workspace, size_t workspace_bytes, size_t need_bytes, uint64_t* pair_bound, uint64_t* zeroed,
                             hipStream_t s) {
    const std::string op = "ma_op_pc_" + name;
    if (!(radius / (double)g.cell <= (double)pcr::MAX_RINGS_RATIO)) throw MaError(MA_ERR_INVALID, op + ": " + what + " / cell must be at most 8");
    volatile float rf = (float)radius;
    volatile float r2 = rf * rf;
    const int R = pcr::rings(rf, g.cell);
    if (!pcr::rings_suffice(g, r2, R))
        throw MaError(MA_ERR_INVALID, op + ": the float32 faces of this grid do not separate cells " + std::to_string(R) +
                                          " apart by more than the radius (origin too large against cell): the pair bound would not hold");
    if (workspace_bytes < need_bytes) throw MaError(MA_ERR_INVALID, op + ": workspace smaller than ma_pc_" + name + "_workspace_bytes(N, nx, ny, nz)");
    const uint64_t cap = max_pairs ? max_pairs : MA_PC_CLUSTER_MAX_PAIRS;
    if (zeroed) *zeroed = 0;
    HIP_CHECK(pcr::launch_bound(ref, N, ref_ld, g, R, workspace, s));
    unsigned long long total = 0;
    HIP_CHECK(hipMemcpyAsync(&total, pcr::total_of(N, g, workspace), sizeof(total), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (pair_bound) *pair_bound = total;
    if (total > cap)
        throw MaError(MA_ERR_INVALID, op + ": the pair bound " + std::to_string(total) + " exceeds max_pairs " + std::to_string(cap) +
                                          ": use a smaller radius or fewer points");
    return r2;
}

// ---- Euclidean clustering over the cell grid (csrc/pc_cluster.hpp) ------------------------------------------------------------------------
size_t ma_pc_cluster_workspace_bytes(int N, int nx, int ny, int nz) { return pc_radius_shape_ok(N, nx, ny, nz) ? pcc::layout(N, nx * ny * nz).bytes : 0; }

int ma_op_pc_cluster(const float* ref, int N, int ref_ld, float radius, const float* origin, float cell, const int32_t* dims, uint64_t max_pairs,
                     int32_t* labels, int32_t* sizes, uint64_t* pairs_bound, void* workspace, size_t workspace_bytes, void* stream) {
    return guarded(nullptr, [&] {
        if (!ref || !origin || !dims || !labels || !workspace) throw MaError(MA_ERR_INVALID, "ma_op_pc_cluster: null pointer");
        const pcg::Grid g = radius_grid("ma_op_pc_cluster", N, origin, cell, dims);
        if (ref_ld != 3 && ref_ld != 6) throw MaError(MA_ERR_INVALID, "ma_op_pc_cluster: ref_ld must be 3 or 6");
        if (!std::isfinite(radius) || !(radius > 0.f)) throw MaError(MA_ERR_INVALID, "ma_op_pc_cluster: radius must be finite and > 0");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        const float r2 = radius_prologue("cluster", "radius", ref, N, ref_ld, g, (double)radius, max_pairs, workspace, workspace_bytes,
                                         pcc::layout(N, pcg::cells_of(g)).bytes, pairs_bound, nullptr, s);
        HIP_CHECK(pcc::launch_hook_flatten(N, r2, g, labels, sizes, workspace, s));
    });
}

// ---- moving-least-squares smoothing over the cell grid (csrc/pc_smooth.hpp) -----------------------------------------------------------------
size_t ma_pc_smooth_workspace_bytes(int N, int nx, int ny, int nz) { return pc_radius_shape_ok(N, nx, ny, nz) ? pcr::layout(N, nx * ny * nz).bytes : 0; }

int ma_op_pc_smooth(const float* ref, int N, int ref_ld, float radius, const float* origin, float cell, const int32_t* dims, int min_count,
                    uint64_t max_pairs, double* moved, double* normals, double* eigvals, int32_t* count, uint64_t* pair_bound, void* workspace,
                    size_t workspace_bytes, void* stream) {
    return guarded(nullptr, [&] {
        if (!ref || !origin || !dims || !workspace) throw MaError(MA_ERR_INVALID, "ma_op_pc_smooth: null pointer");
        if (!moved && !normals && !eigvals && !count)
            throw MaError(MA_ERR_INVALID, "ma_op_pc_smooth: no output: give at least one of moved, normals, eigvals and count");
        const pcg::Grid g = radius_grid("ma_op_pc_smooth", N, origin, cell, dims);
        if (ref_ld != 3 && ref_ld != 6) throw MaError(MA_ERR_INVALID, "ma_op_pc_smooth: ref_ld must be 3 or 6");
        if (!std::isfinite(radius) || !(radius > 0.f)) throw MaError(MA_ERR_INVALID, "ma_op_pc_smooth: radius must be finite and > 0");
        if (min_count < pcs::MIN_COUNT) throw MaError(MA_ERR_INVALID, "ma_op_pc_smooth: min_count must be at least 3, the points a plane takes");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        const float r2 = radius_prologue("smooth", "radius", ref, N, ref_ld, g, (double)radius, max_pairs, workspace, workspace_bytes,
                                         pcr::layout(N, pcg::cells_of(g)).bytes, pair_bound, nullptr, s);
        HIP_CHECK(pcs::launch_smooth(N, r2, g, min_count, moved, normals, eigvals, count, workspace, s));
    });
}

// ---- upsampling: lattice points in every row's plane, kept where the row is the nearest (csrc/pc_upsample.hpp) ------------------------------
static_assert(MA_PC_UPSAMPLE_MAX_M == pcu::MAX_M, "the header's limit is the kernels'");
size_t ma_pc_upsample_workspace_bytes(int N, int nx, int ny, int nz) { return pc_radius_shape_ok(N, nx, ny, nz) ? pcu::layout(N, nx * ny * nz).bytes : 0; }

int ma_op_pc_upsample(const float* ref, int N, int ref_ld, const double* normals, const uint8_t* active, int m, double step, const float* origin, float cell,
                      const int32_t* dims, uint64_t max_pairs, int32_t* counts, float* out_xyz, int32_t* out_seed, uint64_t capacity, uint64_t* total,
                      uint64_t* pair_bound, void* workspace, size_t workspace_bytes, void* stream) {
    return guarded(nullptr, [&] {
        if (!ref || !normals || !origin || !dims || !total || !workspace) throw MaError(MA_ERR_INVALID, "ma_op_pc_upsample: null pointer");
        if (!out_xyz && out_seed) throw MaError(MA_ERR_INVALID, "ma_op_pc_upsample: out_seed without out_xyz: a count-only call takes neither");
        const pcg::Grid g = radius_grid("ma_op_pc_upsample", N, origin, cell, dims);
        if (ref_ld < 3) throw MaError(MA_ERR_INVALID, "ma_op_pc_upsample: ref_ld must be at least 3");
        if (m < 1 || m > pcu::MAX_M) throw MaError(MA_ERR_INVALID, "ma_op_pc_upsample: m must be in 1..64");
        if ((int64_t)N * (2 * m + 1) * (2 * m + 1) > pcu::MAX_SLOTS)
            throw MaError(MA_ERR_INVALID, "ma_op_pc_upsample: N * (2m+1)^2 must be at most 2^31");
        volatile float radius = (float)((double)m * step);
        if (!std::isfinite(step) || !(step > 0.0) || !std::isfinite(radius) || !(radius > 0.f))
            throw MaError(MA_ERR_INVALID, "ma_op_pc_upsample: step must be finite and > 0, and m * step a positive finite float32");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        radius_prologue("upsample", "m * step", ref, N, ref_ld, g, (double)m * step, max_pairs, workspace, workspace_bytes,
                        pcu::layout(N, pcg::cells_of(g)).bytes, pair_bound, total, s);
        HIP_CHECK(pcu::launch_count(ref, N, ref_ld, normals, active, m, step, g, out_xyz ? nullptr : counts, workspace, s));
        long long kept = 0;
        HIP_CHECK(hipMemcpyAsync(&kept, pcu::offs_of(N, g, workspace) + N, sizeof(kept), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        *total = (uint64_t)kept;
        if (!out_xyz) return;                                       // count only
        if ((uint64_t)kept > (uint64_t)MA_PC_GRID_MAX_POINTS - (uint64_t)N)
            throw MaError(MA_ERR_INVALID, "ma_op_pc_upsample: the total " + std::to_string(kept) + " exceeds 2^22 - N = " +
                                              std::to_string(MA_PC_GRID_MAX_POINTS - N) + ": use a smaller m or radius");
        if ((uint64_t)kept > capacity)
            throw MaError(MA_ERR_INVALID, "ma_op_pc_upsample: the total " + std::to_string(kept) + " exceeds the capacity " + std::to_string(capacity) +
                                              " of out_xyz / out_seed: nothing was written");
        HIP_CHECK(pcu::launch_emit(ref, N, ref_ld, normals, active, m, step, g, counts, out_xyz, out_seed, (int64_t)capacity, workspace, s));
    });
}

// ---- dominant planes: hypothesis scoring and one plane applied (csrc/pc_plane.hpp) ----------------------------------------------------------
static bool pc_plane_shape_ok(int N, int H) { return N >= 3 && N <= MA_PC_PLANE_MAX_POINTS && H >= 1 && H <= MA_PC_PLANE_MAX_HYPOTHESES; }

size_t ma_pc_plane_workspace_bytes(int N, int H) { return pc_plane_shape_ok(N, H) ? pcp::layout(N, H).bytes : 0; }

int ma_op_pc_plane_score(const float* ref, int N, int ref_ld, const int32_t* tri, int H, float threshold, float* planes, int32_t* counts, int32_t* best,
                         void* workspace, size_t workspace_bytes, void* stream) {
    return guarded(nullptr, [&] {
        if (!ref || !tri || !counts || !best || !workspace) throw MaError(MA_ERR_INVALID, "ma_op_pc_plane_score: null pointer");
        if (!pc_plane_shape_ok(N, H)) throw MaError(MA_ERR_INVALID, "ma_op_pc_plane_score: need 3 <= N <= 2^22 and 1 <= H <= 2^16");
        if (ref_ld != 3 && ref_ld != 6) throw MaError(MA_ERR_INVALID, "ma_op_pc_plane_score: ref_ld must be 3 or 6");
        if (!std::isfinite(threshold) || !(threshold > 0.f)) throw MaError(MA_ERR_INVALID, "ma_op_pc_plane_score: threshold must be finite and > 0");
        if (workspace_bytes < pcp::layout(N, H).bytes)
            throw MaError(MA_ERR_INVALID, "ma_op_pc_plane_score: workspace smaller than ma_pc_plane_workspace_bytes(N, H)");
        volatile float t2 = threshold * threshold;
        HIP_CHECK(pcp::launch_score(ref, N, ref_ld, tri, H, t2, planes, counts, best, workspace, reinterpret_cast<hipStream_t>(stream)));
    });
}

int ma_op_pc_plane_apply(const float* ref, int N, int ref_ld, const float* plane, float threshold, uint8_t* mask, int32_t* count, double* moments,
                         void* workspace, size_t workspace_bytes, void* stream) {
    return guarded(nullptr, [&] {
        if (!ref || !plane || !workspace) throw MaError(MA_ERR_INVALID, "ma_op_pc_plane_apply: null pointer");
        if (!mask && !count && !moments) throw MaError(MA_ERR_INVALID, "ma_op_pc_plane_apply: at least one of mask, count and moments must be given");
        if (!pc_plane_shape_ok(N, 1)) throw MaError(MA_ERR_INVALID, "ma_op_pc_plane_apply: need 3 <= N <= 2^22");
        if (ref_ld != 3 && ref_ld != 6) throw MaError(MA_ERR_INVALID, "ma_op_pc_plane_apply: ref_ld must be 3 or 6");
        if (!std::isfinite(threshold) || !(threshold > 0.f)) throw MaError(MA_ERR_INVALID, "ma_op_pc_plane_apply: threshold must be finite and > 0");
        if (workspace_bytes < pcp::layout(N, 1).bytes)
            throw MaError(MA_ERR_INVALID, "ma_op_pc_plane_apply: workspace smaller than ma_pc_plane_workspace_bytes(N, 1)");
        volatile float t2 = threshold * threshold;
        const pcp::Plane pl{plane[0], plane[1], plane[2], plane[3], plane[4], plane[5], pcp::plane_rhs(plane[3], plane[4], plane[5], t2)};
        HIP_CHECK(pcp::launch_apply(ref, N, ref_ld, pl, mask, count, moments, workspace, reinterpret_cast<hipStream_t>(stream)));
    });
}

// ---- the tightest box: extents, volumes and the best of up to 2^16 rotations (csrc/pc_align.hpp) -------------------------------------------
static bool pc_align_shape_ok(int N, int H) { return N >= 1 && N <= MA_PC_ALIGN_MAX_POINTS && H >= 1 && H <= MA_PC_ALIGN_MAX_HYPOTHESES; }

size_t ma_pc_align_workspace_bytes(int N, int H) { return pc_align_shape_ok(N, H) ? pca::layout(N, H).bytes : 0; }

int ma_op_pc_align_extents(const float* ref, int N, int ref_ld, const float* centre, const float* rot, int H, float* extents, double* volumes,
                           int32_t* best, void* workspace, size_t workspace_bytes, void* stream) {
    return guarded(nullptr, [&] {
        if (!ref || !centre || !rot || !workspace) throw MaError(MA_ERR_INVALID, "ma_op_pc_align_extents: null pointer");
        if (!extents && !volumes && !best) throw MaError(MA_ERR_INVALID, "ma_op_pc_align_extents: at least one of extents, volumes and best must be given");
        if (!pc_align_shape_ok(N, H)) throw MaError(MA_ERR_INVALID, "ma_op_pc_align_extents: need 1 <= N <= 2^22 and 1 <= H <= 2^16");
        if (ref_ld != 3 && ref_ld != 6) throw MaError(MA_ERR_INVALID, "ma_op_pc_align_extents: ref_ld must be 3 or 6");
        if (workspace_bytes < pca::layout(N, H).bytes)
            throw MaError(MA_ERR_INVALID, "ma_op_pc_align_extents: workspace smaller than ma_pc_align_workspace_bytes(N, H)");
        HIP_CHECK(pca::launch_extents(ref, N, ref_ld, centre, rot, H, extents, volumes, best, workspace, reinterpret_cast<hipStream_t>(stream)));
    });
}

// ---- voxel thinning: one surviving row per occupied voxel, through a hash table on the device (csrc/pc_voxel.hpp) ---------------------------
static bool pc_voxel_capacity_ok(uint64_t capacity) {
    return capacity >= 2 && capacity <= 2 * (uint64_t)MA_PC_VOXEL_MAX_VOXELS && (capacity & (capacity - 1)) == 0;
}

size_t ma_pc_voxel_table_bytes(uint64_t capacity) { return pc_voxel_capacity_ok(capacity) ? pcv::table_bytes(capacity) : 0; }

int ma_op_pc_voxel_reset(void* table, uint64_t capacity, void* stream) {
    return guarded(nullptr, [&] {
        if (!table) throw MaError(MA_ERR_INVALID, "ma_op_pc_voxel_reset: null pointer");
        if (!pc_voxel_capacity_ok(capacity)) throw MaError(MA_ERR_INVALID, "ma_op_pc_voxel_reset: capacity must be a power of two in 2..2^23");
        HIP_CHECK(pcv::launch_reset(table, capacity, reinterpret_cast<hipStream_t>(stream)));
    });
}

int ma_op_pc_voxel_insert(const float* ref, int n, int ref_ld, int64_t row0, const float* origin, float leaf, void* table, uint64_t capacity, void* stream) {
    return guarded(nullptr, [&] {
        if (!ref || !origin || !table) throw MaError(MA_ERR_INVALID, "ma_op_pc_voxel_insert: null pointer");
        if (n < 1 || n > MA_PC_VOXEL_MAX_CHUNK) throw MaError(MA_ERR_INVALID, "ma_op_pc_voxel_insert: need 1 <= n <= 2^22 rows in one call");
        if (row0 < 0 || row0 > (int64_t)MA_PC_VOXEL_MAX_POINTS - n)
            throw MaError(MA_ERR_INVALID, "ma_op_pc_voxel_insert: need row0 >= 0 and row0 + n <= 2^28 rows in all");
        if (ref_ld != 3 && ref_ld != 6) throw MaError(MA_ERR_INVALID, "ma_op_pc_voxel_insert: ref_ld must be 3 or 6");
        if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]))
            throw MaError(MA_ERR_INVALID, "ma_op_pc_voxel_insert: origin must be finite");
        if (!std::isfinite(leaf) || !(leaf > 0.f)) throw MaError(MA_ERR_INVALID, "ma_op_pc_voxel_insert: leaf must be finite and > 0");
        if (!pc_voxel_capacity_ok(capacity)) throw MaError(MA_ERR_INVALID, "ma_op_pc_voxel_insert: capacity must be a power of two in 2..2^23");
        const pcv::Grid g{origin[0], origin[1], origin[2], leaf};
        HIP_CHECK(pcv::launch_insert(ref, n, ref_ld, (uint64_t)row0, g, table, capacity, reinterpret_cast<hipStream_t>(stream)));
    });
}

int ma_op_pc_voxel_mark(void* table, uint64_t capacity, uint8_t* keep, int64_t N, uint32_t* state_out, void* stream) {
    return guarded(nullptr, [&] {
        if (!table || !keep || !state_out) throw MaError(MA_ERR_INVALID, "ma_op_pc_voxel_mark: null pointer");
        if (!pc_voxel_capacity_ok(capacity)) throw MaError(MA_ERR_INVALID, "ma_op_pc_voxel_mark: capacity must be a power of two in 2..2^23");
        if (N < 1 || N > (int64_t)MA_PC_VOXEL_MAX_POINTS) throw MaError(MA_ERR_INVALID, "ma_op_pc_voxel_mark: need 1 <= N <= 2^28 rows");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        HIP_CHECK(pcv::launch_mark(table, capacity, keep, (uint64_t)N, s));
        HIP_CHECK(hipMemcpyAsync(state_out, pcv::state_of(table, capacity), pcv::STATE_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

// ---- rigid registration: one ICP iteration of a source cloud onto a target cloud over the cell grid (csrc/pc_register.hpp) ------------------
static_assert(MA_PC_REGISTER_SUMS == pcreg::SLOTS && MA_PC_REGISTER_THREADS == pcreg::THREADS && MA_PC_REGISTER_ROWS_PER_THREAD == pcreg::ROWS_PER_THREAD,
              "the header's constants are the kernels'");
static bool pc_register_shape_ok(int N, int M, int nx, int ny, int nz) { return pc_radius_shape_ok(N, nx, ny, nz) && M >= 1 && M <= MA_PC_GRID_MAX_POINTS; }

size_t ma_pc_register_workspace_bytes(int N, int M, int nx, int ny, int nz) {
    return pc_register_shape_ok(N, M, nx, ny, nz) ? pcreg::layout(N, M, nx * ny * nz).bytes : 0;
}

// the checks both calls share -> the grid
static pcg::Grid register_grid(const std::string& op, const float* target, int N, int target_ld, const float* source, int M, int source_ld, const float* origin,
                               float cell, const int32_t* dims, void* workspace, size_t workspace_bytes) {
    if (!target || !source || !origin || !dims || !workspace) throw MaError(MA_ERR_INVALID, op + ": null pointer");
    const pcg::Grid g = checked_grid(op, N >= 1 && N <= MA_PC_GRID_MAX_POINTS && M >= 1 && M <= MA_PC_GRID_MAX_POINTS, "1 <= N <= 2^22, 1 <= M <= 2^22", origin, cell, dims);
    if ((target_ld != 3 && target_ld != 6) || (source_ld != 3 && source_ld != 6)) throw MaError(MA_ERR_INVALID, op + ": target_ld and source_ld must be 3 or 6");
    if (workspace_bytes < pcreg::layout(N, M, pcg::cells_of(g)).bytes)
        throw MaError(MA_ERR_INVALID, op + ": workspace smaller than ma_pc_register_workspace_bytes(N, M, nx, ny, nz)");
    return g;
}

int ma_op_pc_register_build(const float* target, int N, int target_ld, const float* source, int M, int source_ld, const float* origin, float cell,
                            const int32_t* dims, void* workspace, size_t workspace_bytes, void* stream) {
    return guarded(nullptr, [&] {
        const pcg::Grid g = register_grid("ma_op_pc_register_build", target, N, target_ld, source, M, source_ld, origin, cell, dims, workspace, workspace_bytes);
        HIP_CHECK(pcreg::launch_build(target, N, target_ld, source, M, source_ld, g, workspace, reinterpret_cast<hipStream_t>(stream)));
    });
}

int ma_op_pc_register_step(const float* target, int N, int target_ld, const float* source, int M, int source_ld, const float* origin, float cell,
                           const int32_t* dims, const float* pose, const float* centre, float max_dist, const float* target_normals, int normals_ld,
                           uint64_t max_pairs, int32_t* nn_idx, float* nn_d2, uint64_t* pair_bound, double* sums, void* workspace, size_t workspace_bytes,
                           void* stream) {
    return guarded(nullptr, [&] {
        const std::string op = "ma_op_pc_register_step";
        const pcg::Grid g = register_grid(op, target, N, target_ld, source, M, source_ld, origin, cell, dims, workspace, workspace_bytes);
        if (!pose || !centre) throw MaError(MA_ERR_INVALID, op + ": null pointer");
        if (!nn_idx && !nn_d2 && !sums) throw MaError(MA_ERR_INVALID, op + ": no output: give at least one of nn_idx, nn_d2 and sums");
        if (target_normals && normals_ld < 3) throw MaError(MA_ERR_INVALID, op + ": normals_ld must be at least 3");
        pcreg::Pose P;
        for (int i = 0; i < 12; ++i) {
            if (!std::isfinite(pose[i])) throw MaError(MA_ERR_INVALID, op + ": pose must be finite");
            (i < 9 ? P.r[i] : P.t[i - 9]) = pose[i];
        }
        if (!std::isfinite(centre[0]) || !std::isfinite(centre[1]) || !std::isfinite(centre[2])) throw MaError(MA_ERR_INVALID, op + ": centre must be finite");
        if (!std::isfinite(max_dist) || !(max_dist > 0.f)) throw MaError(MA_ERR_INVALID, op + ": max_dist must be finite and > 0");
        if (!((double)max_dist / (double)g.cell <= (double)pcr::MAX_RINGS_RATIO)) throw MaError(MA_ERR_INVALID, op + ": max_dist / cell must be at most 8");
        volatile float df = max_dist;
        volatile float r2 = df * df;
        if (!std::isfinite(r2)) throw MaError(MA_ERR_INVALID, op + ": max_dist * max_dist must be a finite float32");
        const int R = pcr::rings(df, g.cell);
        if (!pcr::rings_suffice(g, r2, R))
            throw MaError(MA_ERR_INVALID, op + ": the float32 faces of this grid do not separate cells " + std::to_string(R) +
                                              " apart by more than max_dist (origin too large against cell): the pair bound would not hold");
        const uint64_t cap = max_pairs ? max_pairs : MA_PC_CLUSTER_MAX_PAIRS;
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        HIP_CHECK(pcreg::launch_bound(source, M, source_ld, P, N, g, R, workspace, s));
        unsigned long long total = 0;
        HIP_CHECK(hipMemcpyAsync(&total, pcreg::total_of(N, M, g, workspace), sizeof(total), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (pair_bound) *pair_bound = total;
        if (total > cap)
            throw MaError(MA_ERR_INVALID, op + ": the pair bound " + std::to_string(total) + " exceeds max_pairs " + std::to_string(cap) +
                                              ": use a smaller max_dist or fewer points");
        HIP_CHECK(pcreg::launch_step(target, N, target_ld, source, M, source_ld, P, centre, r2, g, target_normals, normals_ld, nn_idx, nn_d2, sums, workspace, s));
    });
}

// ---- coarse registration from unknown poses: feature histograms, their second pass, matching and hypothesis scoring (csrc/pc_coarse.hpp) ------
static_assert(MA_PC_SPFH_BINS == pcf::BINS && MA_PC_SPFH_DESC == pcf::DESC && MA_PC_SPFH_COLS == pcf::COLS && MA_PC_SPFH_MAX_USED == pcf::MAX_USED &&
                  MA_PC_SPFH_MAX_QUERIES == pcf::MAX_QUERIES && MA_PC_COARSE_MAX_KEYPOINTS == pcf::MAX_KEYPOINTS &&
                  MA_PC_COARSE_MAX_HYPOTHESES == pcf::MAX_HYPOTHESES,
              "the header's constants are the kernels'");

size_t ma_pc_spfh_workspace_bytes(int N, int nx, int ny, int nz) { return pc_radius_shape_ok(N, nx, ny, nz) ? pcf::layout(N, nx * ny * nz).bytes : 0; }

int ma_op_pc_spfh(const float* ref, int N, int ref_ld, const float* normals, int normals_ld, float radius, const float* origin, float cell,
                  const int32_t* dims, uint64_t max_pairs, uint32_t* hist, uint64_t* pair_bound, uint32_t* most_used, void* workspace,
                  size_t workspace_bytes, void* stream) {
    return guarded(nullptr, [&] {
        if (!ref || !normals || !origin || !dims || !hist || !workspace) throw MaError(MA_ERR_INVALID, "ma_op_pc_spfh: null pointer");
        const pcg::Grid g = radius_grid("ma_op_pc_spfh", N, origin, cell, dims);
        if (ref_ld != 3 && ref_ld != 6) throw MaError(MA_ERR_INVALID, "ma_op_pc_spfh: ref_ld must be 3 or 6");
        if (normals_ld < 3) throw MaError(MA_ERR_INVALID, "ma_op_pc_spfh: normals_ld must be at least 3");
        if (!std::isfinite(radius) || !(radius > 0.f)) throw MaError(MA_ERR_INVALID, "ma_op_pc_spfh: radius must be finite and > 0");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        const float r2 = radius_prologue("spfh", "radius", ref, N, ref_ld, g, (double)radius, max_pairs, workspace, workspace_bytes,
                                         pcf::layout(N, pcg::cells_of(g)).bytes, pair_bound, nullptr, s);
        HIP_CHECK(pcf::launch_spfh(N, normals, normals_ld, r2, g, hist, workspace, s));
        unsigned most = 0;
        HIP_CHECK(hipMemcpyAsync(&most, pcf::most_of(N, g, workspace), sizeof(most), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (most_used) *most_used = most;
        if (most > pcf::MAX_USED)
            throw MaError(MA_ERR_INVALID, "ma_op_pc_spfh: a row has " + std::to_string(most) + " neighbours, more than " + std::to_string(pcf::MAX_USED) +
                                              ": thin the cloud (--voxel_size) or use a smaller radius");
    });
}

int ma_op_pc_spfh_gather(const float* ref, int N, int ref_ld, float radius, const float* origin, float cell, const int32_t* dims, uint64_t max_pairs,
                         const uint32_t* hist, const int32_t* query, int Q, uint32_t* desc, uint64_t* pair_bound, void* workspace, size_t workspace_bytes,
                         void* stream) {
    return guarded(nullptr, [&] {
        if (!ref || !origin || !dims || !hist || !query || !desc || !workspace) throw MaError(MA_ERR_INVALID, "ma_op_pc_spfh_gather: null pointer");
        const pcg::Grid g = radius_grid("ma_op_pc_spfh_gather", N, origin, cell, dims);
        if (ref_ld != 3 && ref_ld != 6) throw MaError(MA_ERR_INVALID, "ma_op_pc_spfh_gather: ref_ld must be 3 or 6");
        if (Q < 1 || Q > MA_PC_SPFH_MAX_QUERIES) throw MaError(MA_ERR_INVALID, "ma_op_pc_spfh_gather: need 1 <= Q <= 2^20");
        if (!std::isfinite(radius) || !(radius > 0.f)) throw MaError(MA_ERR_INVALID, "ma_op_pc_spfh_gather: radius must be finite and > 0");
        if (workspace_bytes < pcf::layout(N, pcg::cells_of(g)).bytes)      // the one workspace of both passes: the prologue's wording would name no function
            throw MaError(MA_ERR_INVALID, "ma_op_pc_spfh_gather: workspace smaller than ma_pc_spfh_workspace_bytes(N, nx, ny, nz)");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        const float r2 = radius_prologue("spfh_gather", "radius", ref, N, ref_ld, g, (double)radius, max_pairs, workspace, workspace_bytes,
                                         pcf::layout(N, pcg::cells_of(g)).bytes, pair_bound, nullptr, s);
        HIP_CHECK(pcf::launch_gather(ref, N, ref_ld, r2, g, hist, query, Q, desc, workspace, s));
    });
}

int ma_op_pc_desc_match(const uint32_t* A, int Ka, const uint32_t* B, int Kb, int32_t* idx, float* dist, void* stream) {
    return guarded(nullptr, [&] {
        if (!A || !B || !idx) throw MaError(MA_ERR_INVALID, "ma_op_pc_desc_match: null pointer");
        if (Ka < 1 || Ka > MA_PC_COARSE_MAX_KEYPOINTS || Kb < 1 || Kb > MA_PC_COARSE_MAX_KEYPOINTS)
            throw MaError(MA_ERR_INVALID, "ma_op_pc_desc_match: need 1 <= Ka, Kb <= 4096");
        HIP_CHECK(pcf::launch_match(A, Ka, B, Kb, idx, dist, reinterpret_cast<hipStream_t>(stream)));
    });
}

int ma_op_pc_pose_score(const float* poses, int H, const float* P, const float* Q, int C, float max_dist, int32_t* counts, int32_t* best, void* stream) {
    return guarded(nullptr, [&] {
        if (!poses || !P || !Q || !counts) throw MaError(MA_ERR_INVALID, "ma_op_pc_pose_score: null pointer");
        if (H < 1 || H > MA_PC_COARSE_MAX_HYPOTHESES || C < 1 || C > MA_PC_COARSE_MAX_KEYPOINTS)
            throw MaError(MA_ERR_INVALID, "ma_op_pc_pose_score: need 1 <= H <= 2^16 and 1 <= C <= 4096");
        if (!std::isfinite(max_dist) || !(max_dist > 0.f)) throw MaError(MA_ERR_INVALID, "ma_op_pc_pose_score: max_dist must be finite and > 0");
        volatile float tf = max_dist;
        volatile float t2 = tf * tf;
        if (!std::isfinite(t2)) throw MaError(MA_ERR_INVALID, "ma_op_pc_pose_score: max_dist * max_dist must be a finite float32");
        HIP_CHECK(pcf::launch_score(poses, H, P, Q, C, t2, counts, best, reinterpret_cast<hipStream_t>(stream)));
    });
}

}  // extern "C"
