// PlanOptions (options.h): the one reader of the MTV_* environment, the override record the mtv_debug_* setters write, and the snapshot a
// context takes at creation.  Precedence: override, then environment, then default.  Host code only; needs no device.
#include <mutex>
#include "../../include/mtv_hip_debug.h"
#include "plan_internal.h"

namespace {
// "MT,NT[,KS]" of one kernel family, by the rule the mtv_debug_force_* arguments go through: a tile that does not exist leaves the family off
bool forced_tile(ConvFamily fam, int mt, int nt, int ks, int out[3]) {
    if (fam == CONV_PW && ks == 8) ks = 1;
    if (mt <= 0 || !conv_tile_exists(ConvTile{mt, nt, fam, ks, 0})) return false;
    out[0] = mt; out[1] = nt; out[2] = ks;
    return true;
}
std::string tile_text(const int* v, int n) {
    if (v[0] <= 0) return "0";
    std::string s = std::to_string(v[0]);
    for (int i = 1; i < n; ++i) s += "," + std::to_string(v[i]);
    return s;
}

// One row per variable: its name, how its text sets the field, how the field prints (mtv_debug_options_dump).
struct Row {
    const char* name;
    void (*parse)(PlanOptions& o, const char* e);
    std::string (*print)(const PlanOptions& o);
};
#define ROW(NAME, FIELD, EXPR) {NAME, [](PlanOptions& o, const char* e) { const long v = atol(e); (void)v; o.FIELD = (EXPR); }, [](const PlanOptions& o) { return std::to_string(o.FIELD); }}
#define ROW_TILE(NAME, FIELD, FAM) {NAME, [](PlanOptions& o, const char* e) { int x = 0, y = 0, z = 1; if (sscanf(e, "%d,%d,%d", &x, &y, &z) >= 2) forced_tile(FAM, x, y, z, o.FIELD); }, [](const PlanOptions& o) { return tile_text(o.FIELD, 3); }}
const Row ROWS[] = {
    {"MTV_FORCE_TILE",
     [](PlanOptions& o, const char* e) { int t[4] = {0, 0, 0, 1}; if (sscanf(e, "%d,%d,%d,%d", t, t + 1, t + 2, t + 3) >= 3 && t[0] > 0) { if (t[3] < 1) t[3] = 1; std::copy(t, t + 4, o.force_tile); } },
     [](const PlanOptions& o) { return tile_text(o.force_tile, 4); }},
    ROW_TILE("MTV_FORCE_WIN", force_win, CONV_WIN),
    ROW_TILE("MTV_FORCE_PW", force_pw, CONV_PW),
    ROW_TILE("MTV_FORCE_B3", force_b3, CONV_X3),
    ROW_TILE("MTV_FORCE_LDS", force_lds, CONV_LDS),
    ROW("MTV_FORCE_WIN_XM", force_win_xm, v != 0),
    ROW("MTV_WIN_PACKED", win_packed, v != 0),
    ROW("MTV_WIN_XM", win_xm, v < 0 ? -1 : (int)v),
    ROW("MTV_PW_XM", pw_xm, v < 0 ? -1 : (int)v),
    ROW("MTV_AUTOTUNE", autotune, v != 0),
    ROW("MTV_TUNE_SAMPLES", tune_samples, v < 1 ? 1 : (v > 15 ? 15 : (int)v)),
    {"MTV_TUNE_CACHE", [](PlanOptions& o, const char* e) { o.tune_cache = e; }, [](const PlanOptions& o) { return o.tune_cache; }},
    ROW("MTV_GEO", geo, v != 0),
    ROW("MTV_STAMPS", stamps, 1),
    ROW("MTV_DEEP", deep, v != 0),
    ROW("MTV_DEEP_POOL_FOLD", deep_pool_fold, v != 0),
    ROW("MTV_DEEP_NO_ATTN", deep_no_attn, v != 0),
    ROW("MTV_DEEP_NO_BLOCK", deep_no_block, v != 0),
    ROW("MTV_DEEP_BLOCK_ALL", deep_block_all, v != 0),
    ROW("MTV_DEEP_FIN_PASS", deep_fin_pass, v != 0),
    ROW("MTV_DEEP_XM", deep_xm, (int)v),
    ROW("MTV_DEEP_ATTN_QT", deep_attn_qt, v == 2 ? 2 : 1),
    ROW("MTV_DEEP_ATTN_HPW", deep_attn_form, v == 2 ? 2 : 0),
    ROW("MTV_BLOCK_CL", block_cl, (int)v),
    ROW("MTV_BLOCK_RQ", block_rq, (int)v),
    ROW("MTV_BLOCK_MAX_L", block_max_l, (int)v),
    ROW("MTV_BLOCK_MAX_LC", block_max_lc, v),
    ROW("MTV_RESIDENT_CUS", resident_cus, (int)v),
    ROW("MTV_ATT_QW", att_qw, v == 2 ? 2 : (v == 4 ? 4 : 0)),
    ROW("MTV_ATT_KBX", att_kbx, v == 1 ? 1 : 2),
    ROW("MTV_ATT_QB", att_qb, v != 0),
    ROW("MTV_STEPS_PER_GRAPH", steps_per_graph, v < 1 ? 1 : (v > 32 ? 32 : ((v & ~1L) ? (int)(v & ~1L) : 1))),
    ROW("MTV_AE_NO_GEGLU_FUSION", ae_no_geglu_fusion, 1),
};

// What the mtv_debug_* setters hold, for every context of the process created afterwards: a field is unset (-1; resident_cus, tiles: 0) or a value
struct Overrides {
    int deep = -1, deep_opts = -1, deep_attn_form = -1, att_qb = -1, resident_cus = 0;
    int win[3] = {0, 0, 1}, pw[3] = {0, 0, 1}, b3[3] = {0, 0, 1}, lds[3] = {0, 0, 1};
} g_over;
std::mutex g_over_mutex;

int set_forced(int (Overrides::*field)[3], ConvFamily fam, int mt, int nt, int ks, const char* msg) {
    int v[3] = {0, 0, 1};
    if (mt != 0 && !forced_tile(fam, mt, nt, ks, v)) return fail(MTV_ERR_INVALID, msg);
    std::lock_guard<std::mutex> lock(g_over_mutex);
    std::copy(v, v + 3, g_over.*field);
    return MTV_OK;
}
int set_int(int Overrides::*field, int v, int lo, int hi, const char* msg) {
    if (v < lo || v > hi) return fail(MTV_ERR_INVALID, msg);
    std::lock_guard<std::mutex> lock(g_over_mutex);
    g_over.*field = v;
    return MTV_OK;
}
}  // namespace

PlanOptions options_snapshot() {
    PlanOptions o;
    for (const Row& r : ROWS)
        if (const char* e = getenv(r.name)) r.parse(o, e);
    const Overrides v = [] { std::lock_guard<std::mutex> lock(g_over_mutex); return g_over; }();
    if (v.deep >= 0) o.deep = v.deep;
    if (v.deep_opts >= 0) {
        o.deep_no_attn = (v.deep_opts & MTV_DEEP_OPT_NO_FUSED_ATTN) != 0;
        o.deep_no_block = (v.deep_opts & MTV_DEEP_OPT_NO_BLOCK) != 0;
        o.deep_block_all = (v.deep_opts & MTV_DEEP_OPT_BLOCK_ALL) != 0;
        o.deep_fin_pass = (v.deep_opts & MTV_DEEP_OPT_FIN_PASS) != 0;
    }
    if (v.deep_attn_form > 0) o.deep_attn_form = v.deep_attn_form;
    if (v.att_qb >= 0) o.att_qb = v.att_qb;
    if (v.resident_cus > 0) o.resident_cus = v.resident_cus;
    const int* from[] = {v.win, v.pw, v.b3, v.lds};
    int* to[] = {o.force_win, o.force_pw, o.force_b3, o.force_lds};
    for (int i = 0; i < 4; ++i)
        if (from[i][0] > 0) std::copy(from[i], from[i] + 3, to[i]);
    return o;
}

extern "C" {
int mtv_debug_options_dump(const mtv_ctx* ctx, char* buf, int cap) {
    if (!buf || cap < 1) return fail(MTV_ERR_INVALID, "options_dump: no buffer");
    const PlanOptions o = ctx ? ctx->opt : options_snapshot();
    std::string text;
    for (const Row& r : ROWS) text += std::string(r.name) + "=" + r.print(o) + "\n";
    if ((int)text.size() >= cap) return fail(MTV_ERR_INVALID, "options_dump: buffer of " + std::to_string(cap) + " bytes, " + std::to_string(text.size() + 1) + " needed");
    memcpy(buf, text.c_str(), text.size() + 1);
    return MTV_OK;
}
int mtv_debug_deep(int mode) { return set_int(&Overrides::deep, mode, -1, 1, "mode must be -1 (default), 0 (off) or 1 (on)"); }
int mtv_debug_attention_qb(int mode) { return set_int(&Overrides::att_qb, mode, -1, 1, "mode must be -1 (default), 0 (off) or 1 (on)"); }
int mtv_debug_deep_options(int mask) {
    const char* msg = "mask must be -1 (environment / defaults) or a combination of MTV_DEEP_OPT_*";
    if (mask >= 0 && (mask & 7)) return fail(MTV_ERR_INVALID, msg);      // (bits 1, 2, 4: retired variants)
    return set_int(&Overrides::deep_opts, mask, -1, 127, msg);
}
int mtv_debug_deep_attn_form(int form) { return set_int(&Overrides::deep_attn_form, form, -1, 2, "form must be -1 (the rule / MTV_DEEP_ATTN_HPW), 1 (one head per workgroup) or 2 (head groups)"); }
int mtv_debug_resident_cus(int n) { return set_int(&Overrides::resident_cus, n, 0, 4096, "resident CUs must be 0 (the device's count / MTV_RESIDENT_CUS) or a positive count"); }
int mtv_debug_force_b3(int mt, int nt, int ks) { return set_forced(&Overrides::b3, CONV_X3, mt, nt, ks, "no k_conv_x3<MT, NT> of that shape (4,2 8,2 4,4 2,2 4,1 2,1 8,1), or K slices not 1, 2, 4 or 8"); }
int mtv_debug_force_pw_waves(int mt, int ntw, int waves) { return set_forced(&Overrides::pw, CONV_PW, mt, ntw, waves, "k_conv_pw tile must be {1, 2} x {1, 2} with 8 multiplying waves, or {1, 2} x 1 with 6 / 4 / 2"); }
int mtv_debug_force_pw(int mt, int ntw) { return mtv_debug_force_pw_waves(mt, ntw, 1); }
int mtv_debug_force_win_ks(int mt, int nt, int ks) { return set_forced(&Overrides::win, CONV_WIN, mt, nt, ks, "k_conv_win tile must be 1x2, 1x4, 2x2 or 2x4, with 1, 2 or 4 K slices"); }
int mtv_debug_force_win(int mt, int nt) { return mtv_debug_force_win_ks(mt, nt, 1); }
int mtv_debug_force_lds(int wm, int wn) { return set_forced(&Overrides::lds, CONV_LDS, wm, wn, 1, "wave tile must be 2 or 4 by 2, 4 or 8"); }
}  // extern "C"
