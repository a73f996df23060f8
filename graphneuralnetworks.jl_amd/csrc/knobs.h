// knobs.h — the one table of libgnnmp's tuning knobs (perf experiments; not part of the drop-in surface).
// X(NAME, index, default, "meaning"): enum Knob, KNOB_COUNT, the defaults (runtime.hip: g_knobs) and the names are generated from
// this list; gnnmp/knobs.py mirrors it by hand and tests/test_knobs.py pins the two together.  Indices never change:
// GNNMP_KNOBS="k=v" strings, profiles/README.md, LABNOTES.md and tools/harness.c refer to knobs by number.
#pragma once

// clang-format off
#define GNNMP_KNOB_TABLE(X)                                                                                                          \
    X(FORCE_VEC, 0, 0, "0 = auto, else 1|2|4")                                                                                       \
    X(FORCE_LOG2G, 1, -1, "lanes per row group = 2^value: -1 = auto, else 0..6 (pick_log2g).  Kernels with feature tiles honour any "    \
                          "value.  gnnmp_fused_conv_f32 has none (a lane stores its features to the LDS tile once): it answers "     \
                          "GNNMP_EUNSUPPORTED, nothing written, to any forced width other than the one it derives, and the host "    \
                          "layers take propagate + dense.  The one-pass attention kernels and softmax_rows need the whole row in "   \
                          "one group and derive their own (headgeom.h): the knob does not reach them")                               \
    X(UNROLL, 2, 0, "0 = auto (8: measured best on both bench shapes), else 2|4|8")                                                  \
    X(XCD_REMAP, 3, 1, "0 = off, 1 = auto (default: only when the gathered matrix fits the Infinity Cache), 2 = on")                 \
    X(LONG_ROW, 4, 0, "long-row threshold (0 = auto, at most GNNMP_LONG_ROW)")                                                       \
    X(BLOCK_WAVES, 5, 0, "waves per block in the row kernels: 0 = auto (propagate 4, GAT 1), else 1..4")                             \
    X(DENSE_GENERIC, 6, 0, "0 = auto (dense_plan's whole order, dense_route.h), any other value = never dense_wreg, dense_split, "    \
                           "dense_t16 or dense_narrow (the round-1 kernels only); 1 = not the W-resident 32x32x2 kernel either: "     \
                           "K-chunked on every shape")                                                                               \
    X(DENSE_PREFETCH, 7, 17, "W-resident dense kernel scheduling: bit 4 = per-SIMD matrix-pipe token, low 4 bits = start skew of "   \
                             "waves 4-7 in s_sleep(127) units.  Default 17 (token + 1): 0.83 -> 0.72 ms at 2.4M x 100 => 100.  "     \
                             "Bit 5 = turn the cross-tile register prefetch OFF (on by default; its first version spilled, 270 "     \
                             "VGPRs, and was slower: see dense.hip)")                                                                \
    X(GAT_FAST_EXP, 8, 0, "reserved (retired: the one-pass attention kernel always uses v_exp_f32 now, gat_fused.hip gexp)")         \
    X(GRADW_SLABS, 9, 0, "dW kernel: slabs per CU (0 = auto)")                                                                       \
    X(GRADW_RP, 10, 0, "dW kernel: 0 = the 16x16x4 kernel, < 0 = the round-1 32x32x2 kernel (A/B runs)")                             \
    X(GRADW_MIN_ROWS, 11, 0, "dW kernel: rows-per-slab floor (0 = auto: ~3 slabs per CU on small inputs, 512 on large)")             \
    X(DENSE_T16_WAVES, 12, 0, "dense_t16_kernel: waves per block (0 = auto, else 1..16)")                                            \
    X(T16_DEBUG, 13, 0, "GNNMP_EXPERIMENTS builds only (gnnmp_tune refuses a non-zero value otherwise): phase ablation of "          \
                        "dense_t16_kernel / fused_cat_kernel (1 = no stores, 2 = no x loads, ...: the results are garbage), and the " \
                        "variant number of dense_split_kernel")                                                                      \
    X(FUSED_WAVES, 14, 0, "fused_conv_kernel: 0 = auto (as many waves as LDS holds tiles for, <= 16), > 0 = cap, < 0 = never fuse "  \
                          "- read by the host too (gnnmp/layers.py)")                                                                \
    X(ROW_ORDER, 15, 0, "rows by decreasing length in the row kernels that share a wave between rows: 0 = never, 1 = when the "      \
                        "gathered matrix exceeds the Infinity Cache, 2 = always (use_row_order)")                                    \
    X(SOFTMAX_ROWS, 16, 0, "one-pass narrow-row softmax (softmax_rows.hip): 0 = auto, < 0 = the three-step kernels on every row")    \
    X(DENSE_SPLIT, 17, 0, "split-bf16 dense core (msplit.h, dense_split.hip): 0 = auto (on for its shapes), < 0 = the fp32-MFMA "    \
                          "kernels of rounds 1-2 on every shape")                                                                    \
    X(CHAIN, 18, 0, "fused GraphConv chain kernel (graph_chain.hip): 0 = auto, < 0 = never (layer-by-layer path)")                   \
    X(VARIANT, 19, 0, "A/B switches, a bit field of the VARIANT_* constants below (all variants are correct code)")                  \
    X(TGCN, 20, 0, "TGCN recurrence (temporal.hip): 0 = auto (the one-launch kernel for out <= 128), < 0 = the per-step path (dense " \
                   "launches + the step pointwise kernels, every out) - read by the host layer (gnnmp/layers_temporal.py)")          \
    X(EDGE_DOT_GRAD, 21, 0, "adjoint of the per-edge dot product (linkpred.hip): 0 = auto (the fused kernel for D <= 256), < 0 = "   \
                            "two w_mul_xj propagates (plan and transposed plan) plus an add - read by the host (gnnmp/linkpred.py)") \
    X(HETERO, 22, 0, "heterograph aggregation (hetero.hip): 0 = auto (one hetero_rows_kernel launch per layer, and "                 \
                     "HeteroGraphConv's transform-first path), < 0 = the composition: propagate per relation, then the same kernel " \
                     "over identity relations as the combiner, the A/B baseline - read by the host (gnnmp/hetero.py)")               \
    X(CHUNK_SLOTS, 23, 0, "slots per chunk of a split row, read at plan build (plan.hip: plan_chunk_slots): 0 or anything below "    \
                          "16 = the default of 128; the plan's long-row threshold still caps it")
// clang-format on

namespace gnnmp {

enum Knob {
#define GNNMP_KNOB_ENUM(name, index, def, doc) KNOB_##name = index,
    GNNMP_KNOB_TABLE(GNNMP_KNOB_ENUM)
#undef GNNMP_KNOB_ENUM
#define GNNMP_KNOB_ONE(name, index, def, doc) +1
    KNOB_COUNT = 0 GNNMP_KNOB_TABLE(GNNMP_KNOB_ONE)
#undef GNNMP_KNOB_ONE
};

// the bits of KNOB_VARIANT
enum Variant {
    VARIANT_CHAIN_WAVES_MASK = 3,       // a two-bit field:
    VARIANT_CHAIN_8_WAVES = 1,          //   1 = the wave-pair chain kernel with 8 waves a block (default 12)
    VARIANT_SPLIT_SERIAL_TILES = 16,    // dense_split runs its column tiles one after the other
    VARIANT_SPLIT_DIRECT_STORES = 32,   // dense_split stores straight from the accumulator layout (default: the per-wave LDS stage)
    VARIANT_NO_WREG = 64,               // never dense_wreg
    VARIANT_TWO_KERNEL_FOLD = 128,      // split rows folded by a second kernel (csr_combine / gat_fused_combine) as in rounds 1-4
                                        // instead of by the last chunk to arrive inside the row kernel (round 5, use_fold)
    VARIANT_WREG_SMALL = 512,           // dense_wreg from 4 096 rows on (default 32 768: below that its eight-wave blocks are too
                                        // few), so that small tests reach it
};

}  // namespace gnnmp

// GNNMP_EXPERIMENTS (make EXPERIMENTS=1) is the one switch that compiles experiment-only code in: the phase ablations and kernel
// variants behind KNOB_T16_DEBUG, which compute garbage on purpose, and the chain kernel's cycle trace.  In a release build none of
// it can be reached and every knob value selects correct code.
#ifdef GNNMP_EXPERIMENTS
#define GNNMP_ABLATION(bits) (bits)
#else
#define GNNMP_ABLATION(bits) 0
#endif
