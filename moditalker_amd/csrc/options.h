// Every setting that decides which kernel a launch runs, in one record.  A context takes ONE snapshot when it is created (ctx_init_common: defaults,
// then the MTV_* environment, then what the mtv_debug_* setters hold -- options.hip) and never changes its mind: plans read mtv_ctx::opt, launchers get
// the record as a parameter.  README.md "Run-time switches" lists the variables; mtv_debug_options_dump prints a snapshot.  Host only; gfx950 only.
#pragma once
#include <string>

struct PlanOptions {
    int force_tile[4] = {0, 0, 0, 1};   // MTV_FORCE_TILE "MT,NT,NW[,KS]": every conv on that k_conv tile ([0] = 0: off)
    int force_win[3] = {0, 0, 1};       // MTV_FORCE_WIN / mtv_debug_force_win[_ks] "MT,NT[,KS]": every eligible 3x3 conv on k_conv_win
    int force_pw[3] = {0, 0, 1};        // MTV_FORCE_PW / mtv_debug_force_pw[_waves] "MT,NTW[,waves]": every eligible 1x1 conv on k_conv_pw
    int force_b3[3] = {0, 0, 1};        // MTV_FORCE_B3 / mtv_debug_force_b3: every eligible conv on the split-bf16 kernel k_conv_x3
    int force_lds[3] = {0, 0, 1};       // MTV_FORCE_LDS / mtv_debug_force_lds: every eligible conv on the LDS-tiled kernel k_conv_lds
    int force_win_xm = 0;               // MTV_FORCE_WIN_XM: the forced k_conv_win tile with the XCD-aware block order
    int win_packed = 1;                 // MTV_WIN_PACKED: k_conv_win reads its packed weight copy (0: the [krow][ldw] matrix)
    int win_xm = -1, pw_xm = -1;        // MTV_WIN_XM / MTV_PW_XM: block order of every k_conv_win / k_conv_pw launch (-1: the tile's)
    int autotune = 1, tune_samples = 5; // MTV_AUTOTUNE: 0 keeps the analytic pick for shapes the tile table does not list; MTV_TUNE_SAMPLES (1 .. 15)
    std::string tune_cache;             // MTV_TUNE_CACHE: a file that replaces the committed tile table and is appended to
    int geo = 1, stamps = 0;            // MTV_GEO: 0 = gather tables instead of the arithmetic; MTV_STAMPS (diagnostic build: mtv_debug_stamps)
    int deep = 1, deep_pool_fold = 1;   // MTV_DEEP / mtv_debug_deep; MTV_DEEP_POOL_FOLD
    int deep_no_attn = 0, deep_no_block = 0, deep_block_all = 0, deep_fin_pass = 0;   // MTV_DEEP_NO_ATTN ... / mtv_debug_deep_options (MTV_DEEP_OPT_*)
    int deep_xm = 1;                    // MTV_DEEP_XM: 0 = the plain block order in every k_deep_conv launch
    int deep_attn_qt = 1;               // MTV_DEEP_ATTN_QT: 2 = two query tiles x four key parts per k_deep_attn workgroup
    int deep_attn_form = 0;             // MTV_DEEP_ATTN_HPW=2 / mtv_debug_deep_attn_form: 0 the rule, 1 one head per workgroup, 2 head groups
    int block_cl = 0, block_rq = 0, block_max_l = 32;     // MTV_BLOCK_CL / MTV_BLOCK_RQ: k_deep_block's cluster shape (0: configured);
    long block_max_lc = 128L * 256;                       // MTV_BLOCK_MAX_L / MTV_BLOCK_MAX_LC: where k_deep_block is taken
    int resident_cus = 0;               // MTV_RESIDENT_CUS / mtv_debug_resident_cus (0: the device's count)
    int att_qw = 0, att_kbx = 2;        // MTV_ATT_QW: 2 | 4 query tiles per wide k_attention workgroup (0: the rule); MTV_ATT_KBX: 1 = no double key blocks
    int att_qb = -1;                    // MTV_ATT_QB / mtv_debug_attention_qb: QK^T on the bf16 pipe; -1 = where it measures faster (d = 16 / 32)
    int steps_per_graph = 8;            // MTV_STEPS_PER_GRAPH (1, or even up to 32)
    int ae_no_geglu_fusion = 0;         // MTV_AE_NO_GEGLU_FUSION
    bool any_forced_tile() const { return force_tile[0] > 0 || force_win[0] > 0 || force_pw[0] > 0 || force_b3[0] > 0 || force_lds[0] > 0; }
};
// options.hip: what a context created now would get
PlanOptions options_snapshot();
