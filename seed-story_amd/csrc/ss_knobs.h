// Tuning knobs: the one list.  A knob is a process-wide int that selects a kernel, a launch rule or an arithmetic mode; callers
// set it through ss_set_tuning("name", v), the library reads it with knob(K_name).  One row per knob: name, default, what it does.
// A name that is not in this list does not exist: ss_set_tuning refuses it.
#pragma once
#include <limits.h>

#include <atomic>

// X(name, default, description)
#define SS_KNOB_LIST(X)                                                                                                              \
    /* ---- attention ---- */                                                                                                        \
    X(attn_waves, 0, "flash v3p waves per workgroup: 0 = rule by shape, 4 / 8 / 16 = force")                                         \
    X(attn_xcd, 1, "flash v3 / v3p: one XCD owns heads k, k+8, ... (flattened grid) when batch x heads is a multiple of 8")          \
    X(attn_ver, 6, "prefill attention kernel: 6 = v3p without prefetch (hd <= 64), 5 = v3p with prefetch, 3 / 4 = v3 swizzled / "    \
                   "linear V, 2 = v2 (EXPERIMENTAL build only), below = v1")                                                         \
    X(attn_cross64, 0, "EXPERIMENTAL build: contexts of <= 64 keys at head_dim 64 keep K / V in registers (cross_attn64)")           \
    X(attn_decode_nsplit, 0, "decode attention KV splits per (head, slot): 0 = 16 / slots, else rounded up to 4 / 8 / 16 / 32")      \
    /* ---- GEMM ---- */                                                                                                             \
    X(gemm_f32_split, 0, "gate mode: fp32 GEMM / GEMV through split-bf16 MFMA instead of the exact fp32 FMA chain")                  \
    X(gemm_f32_split_order, 16, "gate mode grid: bands of this many N tiles walked M-fastest; 0 = plain N-fastest grid")             \
    X(gemm_f32_split_tile, 0, "gate mode tile: 0 = rule by shape, 1 = 256x128, 2 = 128x256, 3 = 128x128")                            \
    X(gemm_cfg, 0, "force one GEMM tile id for every launch (0 = tile table, then the closed-form rule)")                            \
    X(gemm_table, 1, "consult the per-shape tile table before the closed-form rule")                                                 \
    X(gemm_autotune_log, 0, "print every candidate's time while a shape is tuned")                                                   \
    X(gemm_xcd_swizzle, 8, "tile-id swizzle of the GEMM / conv grids (0 = row-major)")                                               \
    X(gemm_epi_generic, 0, "take the generic epilogue instead of the specialised ones (A/B runs)")                                   \
    X(gemm_rowstat_fallback, 0, "skip the tiles with a statistics epilogue and take the separate-kernel fallback (tests)")           \
    X(lnfold_w4, 0, "EXPERIMENTAL build: LayerNorm-folded GEMM stays on a 4-wave tile instead of the 8-wave reroute")                \
    X(gemm_splitk, 1, "split-K plan for eligible shapes in ss_gemm_splitk")                                                          \
    X(gemm_splitk_s, 0, "force the split-K count (2..8) where the workspace and K allow it; 0 = planned count")                      \
    X(gemm_splitk_swz, 0, "tile-id swizzle of the split-K grid (0 = row-major, the measured best)")                                  \
    X(gemm_fp8_cfg, 0, "force one fp8 GEMM tile id (0 = closed-form rule)")                                                          \
    X(gemm_fp8_swz, KNOB_UNSET, "tile-id swizzle of the fp8 GEMM grid; unset = 8 with 16 or more row tiles, else 0")                 \
    X(gemm_fp8_debug, 0, "print shape, tile id and swizzle of every ss_gemm_fp8 launch")                                             \
    /* ---- elementwise ---- */                                                                                                      \
    X(layernorm_rows_per_wave, 1, "LayerNorm wave kernel at >= 8192 rows: rows per wave (1 | 2 | 4)")                                \
    /* ---- LLaMA engine ---- */                                                                                                     \
    X(llama_graph, 1, "decode tokens replay a captured graph (0 = eager launches)")                                                  \
    X(llama_done_poll, 8, "decode tokens launched between two polls of the done flags")                                              \
    X(llama_batched_attn, 1, "prefill of 2..8 equal-length slots runs one batched attention launch")                                 \
    /* ---- GEMV ---- */                                                                                                             \
    X(gemv_mfma_blocks, 256, "MFMA GEMV forms: workgroups per round of 16-row tiles")                                                \
    X(gemv_mfma_generic, 0, "MFMA GEMV: the generic kernel instead of the exact-K specialisations")                                  \
    X(gemv_mfma_long, 1, "MFMA GEMV: the packed 43-step form for K = 11008")                                                         \
    X(gemv_mfma_nt, 0, "MFMA GEMV: non-temporal weight loads (measured slower)")                                                     \
    X(gemv_max_blocks, 2048, "dot-product GEMV: cap on the workgroup count")                                                         \
    X(gemv_x_reg_packs, 16, "dot-product GEMV: x stays in registers while batch x K iterations <= this many 16-byte packs")          \
    X(gemv_force_lds, 0, "dot-product GEMV: always stage x in LDS")                                                                  \
    X(gemv_nt, 1, "dot-product GEMV: non-temporal weight loads")                                                                     \
    X(gemv_mfma_min_nb, 3, "fewest sequences that take an MFMA GEMV form")                                                           \
    X(gemv_groups_per_wave, 0, "dot-product GEMV: row groups per wave; 0 = ~2.5k waves in all")                                      \
    X(gemv_split_refused, 0, "COUNTER: gate-mode GEMV launches that could not take the split form and ran as exact sweeps")          \
    /* ---- read by the Python host layer only ---- */                                                                               \
    X(vae_fp32, 0, "VAE decode in fp32 whatever the module dtype")                                                                   \
    X(vae_bf16, 0, "fp16 VAE modules decode in bf16 instead of fp32")                                                                \
    X(unet_graph, 1, "denoising steps replay a captured graph")                                                                      \
    X(gemm_autotune, 1, "tune unseen GEMM shapes on first use")                                                                      \
    X(img_block_logits, 1, "image-token blocks also compute the reference's (unused) per-position logits")                           \
    X(img_block_decode, KNOB_UNSET, "forced image-token blocks decode as one block; unset = the SEEDSTORY_IMG_BLOCK environment rule")                \
    X(llama_decode_w8, 0, "LlamaEngine default of decode_weights: 1 = fp8 (e4m3) weight-only decode projections")                \
    X(llama_decode_mx4, 0, "LlamaEngine default of decode_weights: 1 = MXFP4 weight-only decode projections (not with llama_decode_w8)") \
    X(llama_kv8, 0, "LlamaEngine default of kv_cache: 1 = decode attention reads an fp8 (e4m3) shadow of the KV cache")                  \
    X(llama_spec_rows, 0, "LlamaEngine default of speculate: rows (2..8) of a prompt-lookup speculative step of generate; 0 = off") \
    X(sdxl_solver, 0, "SDXL render sampler: 0 = the scheduler object as given, 2 = DPM-Solver++ 2M, 3 = DPM-Solver++ 2M on Karras sigmas")

namespace ss {

constexpr int KNOB_UNSET = INT_MIN;   // default of a knob whose value is decided at the call site until somebody sets it

enum Knob : int {
#define X(name, dflt, doc) K_##name,
    SS_KNOB_LIST(X)
#undef X
    K_COUNT
};

struct KnobInfo { const char* name; int dflt; const char* doc; };
inline constexpr KnobInfo kKnobs[] = {
#define X(name, dflt, doc) {#name, dflt, doc},
    SS_KNOB_LIST(X)
#undef X
};
static_assert(sizeof(kKnobs) / sizeof(kKnobs[0]) == K_COUNT && K_COUNT == 47, "knob list and enum out of step");

extern std::atomic<int> g_knobs[K_COUNT];   // ss_runtime.hip, constant-initialised from the defaults

inline int knob(Knob k) { return g_knobs[k].load(std::memory_order_relaxed); }
inline int knob_or(Knob k, int fallback) { const int v = knob(k); return v == KNOB_UNSET ? fallback : v; }
inline void knob_add(Knob k, int n) { g_knobs[k].fetch_add(n, std::memory_order_relaxed); }   // counters

}  // namespace ss
