// 2D backbone (RPN) + shared head, host side: what a context decides once.  layer_menu (the families' menus composed per layer shape
// and precision), the per-family rules of the tuner and the launcher, the cost model, pack_layer (gathers a layer's weights and hands
// them to the family's packer), the tuner and its cache, and pp_net_create / pp_net_commit / pp_net_destroy.  The types are in
// conv_net.h; its one kernel, fill_pattern, fills the tuner's input.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unistd.h>
#include "conv_net.h"

namespace ppc {

// The tilings a layer may run, composed from what the families export (conv_common.h).  Content and order are part of the plan: the
// order decides menu[0], the tuner's ties and what PP_AUTOTUNE=0 takes, and menu.size() is in the tune-cache key (autotune_layer).
// Tests read the menus back through pp_menu_names and pin entry i of every menu in turn (tests/test_menu_exact_gpu.py): a new entry
// is picked up by those slot tests automatically, as long as the menu stays within their MENU_SLOTS (32) entries -- tests/test_menu_cpu.py
// goes red beyond that.
static void layer_menu(int kind, int stride, int up, std::vector<Variant>& menu, int cin = 0, bool roofline_layer = false, bool head9 = true, int prec = 0,
                bool first_conv = false)
{
    const bool g1ok = cin % 32 == 0; // gemm1x1 runs K in rings of 8 quad-steps without a tail
    // reduced-precision modes (pp_set_precision): the 1x1 contractions -- the three ConvTranspose(k = s) upsamplers and the
    // 9-anchor head -- run their bf16x3 / bf16 / fp16 gemm1x1 tilings, the 3x3 convolutions the 16-bit operand kernels of
    // conv16.hip.  A layer whose shape none of them takes (autotune_layer checks variant_ok / shape_ok) falls back to the
    // fp32 menu below, and pp_layer_tilings shows it.
    if (prec && g1ok && (kind == 1 || (kind == 2 && head9))) {
        gemm1x1_menu(kind, up, prec, menu);
        return;
    }
    if (prec && kind == 0 && cin % 16 == 0) {
        // fp16s: the fp16-operand kernels on fp16 tensors; the first conv reads the fp32 PFN rows / canvas and writes fp16
        if (prec == 4) conv16_menu(stride, 3, menu, first_conv ? 2 : 3);
        else conv16_menu(stride, prec, menu);
        return;
    }
    if (kind == 2) {
        // the persistent 1x1 GEMM's head epilogue (head_tile_row) is laid out for the reference's 9 anchors per location
        if (g1ok && head9) gemm1x1_menu(kind, up, 0, menu);
        conv_direct_menu(kind, stride, up, menu);
    } else if (kind == 1) {
        conv_direct_menu(kind, stride, up, menu);
        if (g1ok) gemm1x1_menu(kind, up, 0, menu);
    } else {
        conv_direct_menu(kind, stride, up, menu);
        if (stride != 2) {
            wino2_menu(menu, roofline_layer);
            wino4_menu(menu, roofline_layer);
            if (cin % 32 == 0) wino6_menu(menu, roofline_layer); // Winograd F(4x4,3x3), 16x16 px (wino6.hip)
        }
    }
}

// strip tilings of wino4 / wino6 (launch_conv): a map that is not a multiple of the main tile (16x16 px) is covered by whole main
// tiles plus a right strip of 4 x 64 px tiles and a bottom strip of 64 x 4 px tiles -- 100 x 100: 36 + 2 + 2 tiles instead of
// 49 mostly-empty ones
const Variant& strip_v(Family f) // 4 px wide, 64 px tall
{
    static const Variant w4 = wino4_strip_v(), w6 = wino6_strip_v();
    return f == Family::Wino6 ? w6 : w4;
}
const Variant& strip_h(Family f) // 64 px wide, 4 px tall
{
    static const Variant w4 = wino4_strip_h(), w6 = wino6_strip_h();
    return f == Family::Wino6 ? w6 : w4;
}

// cost model: wavefronts are dealt to 1024 SIMDs; a SIMD's time ~ (its wave count) x (tile pairs per wave).
static double model_cost(const Variant& v, int rows, int Hout, int Wout)
{
    const double blocks = (double)pp_div_up(Wout, v.pw) * pp_div_up(Hout, v.ph) * pp_div_up(rows, v.bm);
    const double waves = blocks * v.waves;
    double cost = std::ceil(waves / 1024.0) * v.pairs;
    if (waves < 1536.0) cost *= 1.15;          // a lone wave per SIMD cannot hide its own staging
    cost *= 1.0 + 0.02 * (20.0 / v.pairs);     // smaller wave tiles re-read operands more often
    return cost;
}

// ---- the per-family rules of the tuner and the launcher ----
// rows: wino4, conv16 and wino6 tile whole row blocks; the others clip their last block
bool variant_ok(const Variant& v, int rows)
{
    switch (v.family) {
    case Family::Wino4:
    case Family::Conv16:
    case Family::Wino6: return rows % v.bm == 0;
    default: return v.bm <= ((rows + 63) / 64) * 64;
    }
}
// shape limits of a tiling family
bool shape_ok(const Variant& v, int Hin, int Win, int Wout)
{
    switch (v.family) {
    case Family::Wino4: return !(Wout & 1); // float2 row stores (even output width)
    // gemm1x1 feeds four N-tiles from one dwordx4 of 4 consecutive pixels of the input plane (pixel count a multiple of 4 -- a
    // 9 x 11 map has 99); with a 16-bit tensor it has no path for maps that are not a multiple of 4 wide
    case Family::Gemm1x1: return !((Hin * Win) & 3) && !(v.io16 && (Wout & 3));
    // conv16 fetches its patches as aligned pixel quads and stores pixel quads (input and output width multiples of 4)
    case Family::Conv16: return !((Win & 3) || (Wout & 3));
    // wino6 works on whole 4x4 output tiles and dwordx4 rows (maps a multiple of 4 in both directions; stride 1: Hin = Hout)
    case Family::Wino6: return !((Wout & 3) || (Hin & 3));
    default: return true;
    }
}
// LDS bytes of a launch of v on a layer with cin input channels (gemm1x1 keeps the whole [K][BM] weight slab)
size_t layer_lds(const Variant& v, int cin) { return v.family == Family::Gemm1x1 ? g1_lds(v, cin) : v.lds; }
// May tiling v run a layer of `rows` GEMM rows and cin input channels on these maps?  The one statement of the rule: the tuner
// (autotune_layer) and pp_menu_names both ask here.
bool tiling_legal(const Variant& v, int rows, int cin, int Hin, int Win, int Wout)
{
    return variant_ok(v, rows) && shape_ok(v, Hin, Win, Wout) && layer_lds(v, cin) <= (size_t)160 * 1024;
}
// One frame per launch: the families that finalise the producer's statistics in their own prologue, instead of a norm_finalize
// launch in front of the layer -- 14 launches of 4.7 us + a boundary each per frame at batch 1.  (Batched launches keep
// norm_finalize: a persistent workgroup would redo the fp64 finalisation at every frame change.)
bool finalises_in_prologue(Family f)
{
    switch (f) {
    case Family::Direct:
    case Family::Gemm1x1:
    case Family::Wino4:
    case Family::Wino6: return true;
    default: return false;
    }
}
// MFMA flops a tiling executes per algorithmic flop of the direct convolution
double executed_ratio(const Variant& v)
{
    switch (v.family) {
    case Family::Wino6: return 0.25;
    case Family::Wino:
    case Family::Wino4: return 4.0 / 9.0;
    case Family::Conv16: return v.prec == 1 ? 3.0 : 1.0; // bf16x3: three MFMAs per product
    default: return 1.0;
    }
}

static Variant pick_variant(int kind, int stride, int up, int rows, int Hout, int Wout, bool head9 = true)
{
    std::vector<Variant> menu;
    layer_menu(kind, stride, up, menu, 0, false, head9, 0);
    double best = 1e30;
    Variant bv = menu[0];
    for (const Variant& v : menu) {
        if (!variant_ok(v, rows) || (v.family != Family::Direct && v.family != Family::Wino)) continue; // persistent kernels are only chosen by measurement
        const double c = model_cost(v, rows, Hout, Wout);
        if (c < best) { best = c; bv = v; }
    }
    // Without on-device tuning (PP_AUTOTUNE=0) prefer what the tuner settles on for these layer kinds on MI355X;
    // the cost model above only ranks the direct tilings.
    const char* prefer = (kind == 0 && stride == 1) ? "wino tw8 w1x4 bx1 kc8"
                         : (kind == 1 && up == 2)   ? "g1x1 m4 n4 e1"
                         : (kind == 1 && up == 4)   ? "g1x1 m4 n4 e2"
                         : (kind == 2 && head9)     ? "g1x1 m6 n4 e3"
                                                    : nullptr;
    if (prefer)
        for (const Variant& v : menu)
            if (variant_ok(v, rows) && shape_ok(v, Hout, Wout, Wout) && !strcmp(v.name, prefer)) return v;
    return bv;
}

// The layer's weights as [rows][cin][taps] from the host tensors, by layer kind; sets L.rows
static int gather_rows(pp_ctx* ctx, Layer& L, std::vector<float>& w)
{
    auto missing = [&](const std::string& name) { return pp_fail(ctx, PP_E_NAME, ("missing/mis-shaped weight " + name).c_str()); };
    auto it = ctx->host_w.find(L.wkey);
    L.rows = layer_rows(ctx, L);
    if (L.kind == 0) {
        if (it == ctx->host_w.end() || (int64_t)it->second.data.size() != (int64_t)L.cout * L.cin * 9) return missing(L.wkey);
        w = it->second.data; // [cout][cin][3][3]
    } else if (L.kind == 1) {
        const int u2 = L.up * L.up;
        if (it == ctx->host_w.end() || (int64_t)it->second.data.size() != (int64_t)L.cin * L.cout * u2) return missing(L.wkey);
        w.resize((size_t)L.rows * L.cin); // ConvTranspose weight [cin][cout][k][k] -> row (co*u2 + dy*u + dx)
        const std::vector<float>& s = it->second.data;
        for (int ci = 0; ci < L.cin; ++ci)
            for (int co = 0; co < L.cout; ++co)
                for (int d = 0; d < u2; ++d) w[((size_t)co * u2 + d) * L.cin + ci] = s[((size_t)ci * L.cout + co) * u2 + d];
    } else {
        w.assign((size_t)L.rows * L.cin, 0.f);
        int r0 = 0;
        for (const HeadPart& part : kHead) {
            const int cnt = part.rows_per_anchor * ctx->cfg.num_anchor_per_loc;
            auto hw = ctx->host_w.find(part.weight);
            if (hw == ctx->host_w.end() || (int64_t)hw->second.data.size() != (int64_t)cnt * L.cin) return missing(part.weight);
            memcpy(&w[(size_t)r0 * L.cin], hw->second.data.data(), sizeof(float) * cnt * L.cin);
            r0 += cnt;
        }
    }
    return 0;
}

int pack_layer(pp_ctx* ctx, Layer& L, bool index_positions)
{
    const Variant& v = L.var;
    std::vector<float> w, f;  // the gathered weights; an fp32 image
    std::vector<uint16_t> h;  // a 16-bit image
    if (int rc = gather_rows(ctx, L, w)) return rc;
    if (v.family == Family::Wino || v.family == Family::Wino4) wino2_transform(w);
    if (index_positions) // (wino6_pack numbers its own transform's positions)
        for (size_t k = 0; k < w.size(); ++k) w[k] = (float)(k + 1);
    switch (v.family) {
    case Family::Direct: conv_direct_pack(w, L.rows, L.cin, L.kind == 0 ? 9 : 1, v, f); break;
    case Family::Wino: wino2_pack(w, L.rows, L.cin, v, f); break;
    case Family::Wino4: wino4_pack(w, L.rows, L.cin, v, f); break;
    case Family::Wino6: wino6_pack(w.data(), L.rows, L.cin, f, index_positions); break;
    case Family::Conv16: conv16_pack(w, L.rows, L.cin, v, h); break;
    case Family::Gemm1x1:
        if (L.kind == 2) gemm1x1_head_order(w, L.cin);
        if (v.prec) gemm1x1_pack16(w, L.rows, L.cin, v, h);
        else gemm1x1_pack(w, L.rows, L.cin, v, f);
        break;
    }
    // the finished image replaces the layer's device copy
    const void* image = h.empty() ? (const void*)f.data() : (const void*)h.data();
    const size_t bytes = h.empty() ? f.size() * sizeof(float) : h.size() * sizeof(uint16_t);
    if (L.w) (void)hipFree(L.w);
    PP_HIP(hipMalloc((void**)&L.w, bytes));
    L.w_bytes = bytes;
    PP_HIP(hipMemcpy(L.w, image, bytes, hipMemcpyHostToDevice));
    return 0;
}

namespace {
__global__ void __launch_bounds__(256) fill_pattern(float* __restrict__ x, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned h = (unsigned)i * 2654435761u;
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        x[i] = (float)(h & 0xFFFF) * (1.0f / 65536.0f); // [0,1): random-looking, not zeros (zeros raise the clock)
    }
}
} // namespace

// "signature<TAB>tiling" lines of a cache file -> c (a missing file adds nothing)
static void read_cache_file(const char* path, std::map<std::string, std::string>& c)
{
    FILE* f = fopen(path, "r");
    if (!f) return;
    char line[512];
    while (fgets(line, sizeof(line), f)) {
        char* tab = strchr(line, '\t');
        if (!tab) continue;
        *tab = 0;
        char* val = tab + 1;
        val[strcspn(val, "\r\n")] = 0;
        c[line] = val;
    }
    fclose(f);
}

std::map<std::string, std::string>& tune_cache()
{
    // layer signature -> variant name, per process; PP_TUNE_CACHE=<file> persists it across processes
    static std::map<std::string, std::string> c;
    static bool loaded = false;
    if (!loaded) {
        loaded = true;
        if (const char* path = getenv("PP_TUNE_CACHE")) read_cache_file(path, c);
    }
    return c;
}

// Merge with what other processes wrote meanwhile, write to a temp file, rename() over the target: concurrent ranks can
// neither tear the file nor drop each other's entries (the last rename wins with a superset of what it read).
static void tune_cache_save()
{
    const char* path = getenv("PP_TUNE_CACHE");
    if (!path) return;
    std::map<std::string, std::string> merged;
    read_cache_file(path, merged);
    for (auto& kv : tune_cache()) merged[kv.first] = kv.second;
    char tmp[1024];
    snprintf(tmp, sizeof(tmp), "%s.tmp.%d", path, (int)getpid());
    if (FILE* f = fopen(tmp, "w")) {
        for (auto& kv : merged) fprintf(f, "%s\t%s\n", kv.first.c_str(), kv.second.c_str());
        fclose(f);
        if (rename(tmp, path) != 0) remove(tmp);
    }
}

constexpr int TUNE_FRAMES = 16; // frames per timed launch of the tuner (half the default bench pass of 32; the picks do not change beyond 16)
static int tune_frames(const pp_ctx* ctx) { return ctx->max_batch < TUNE_FRAMES ? ctx->max_batch : TUNE_FRAMES; }

// Milliseconds per launch over `reps` launches on the null stream, after one warm-up launch.  Owns its two events on every path.
template <typename Launch>
static int time_launches(pp_ctx* ctx, int reps, Launch&& launch, double& out_ms)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto run = [&]() -> int {
        PP_HIP(hipEventCreate(&e0));
        PP_HIP(hipEventCreate(&e1));
        for (int it = 0; it <= reps; ++it) {
            if (it == 1) PP_HIP(hipEventRecord(e0, 0));
            if (int rc = launch()) return rc;
        }
        float ms = 0.f;
        PP_HIP(hipEventRecord(e1, 0));
        PP_HIP(hipEventSynchronize(e1));
        PP_HIP(hipEventElapsedTime(&ms, e0, e1));
        out_ms = ms / reps;
        return 0;
    };
    const int rc = run();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return rc;
}

// Measure every tiling of `legal` on the device and keep the fastest in L.var.  Weights are really packed for each candidate, the
// prologue / statistics epilogue run as in production.
static int time_layer(pp_ctx* ctx, Layer& L, const std::vector<Variant>& legal, const char* sig, const ConvCall& shape, bool verbose)
{
    pp_net* net = (pp_net*)ctx->net;
    ConvCall call = shape;
    if (L.kind == 2 || (L.kind == 0 && L.stride == 1)) { call.pre.mode = PRE_AFFINE; call.pre.scale = net->ones; call.pre.shift = net->zeros; }
    call.stat = (ctx->cfg.norm_kind == 0 && L.kind != 2) ? net->stats + (size_t)23 * NREP * 320 * 2 : nullptr;
    call.stat_C = (L.kind == 1) ? 320 : L.cout;
    if (L.kind == 2) { call.out = ctx->f_cls; call.out_box = ctx->f_box; call.out_dir = ctx->f_dir; }
    // batched like production, every frame with its own buffers: a launch then streams more than the 256 MB
    // Infinity Cache holds, as in production (aliased frames would hide a tiling's HBM re-reads)
    call.nb = tune_frames(ctx);
    auto time_variant = [&](const Variant& v, int reps, double& out_ms) -> int {
        const size_t need = layer_lds(v, L.cin);
        L.var = v;
        PP_HIP(hipFuncSetAttribute((const void*)v.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need));
        if (v.kern2) PP_HIP(hipFuncSetAttribute((const void*)v.kern2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need));
        if (int rc = pack_layer(ctx, L)) return rc;
        return time_launches(ctx, reps, [&] { return launch_conv(ctx, L, call, 0); }, out_ms);
    };
    // pass 1: every legal tiling, 3 timed launches
    std::vector<std::pair<double, const Variant*>> timed;
    for (const Variant& v : legal) {
        double ms;
        if (int rc = time_variant(v, 3, ms)) return rc;
        if (verbose) fprintf(stderr, "[pp autotune] %-28s %-34s %8.1f us\n", sig, v.name, ms * 1e3);
        timed.push_back({ms, &v});
    }
    if (timed.empty()) return pp_fail(ctx, PP_E_STATE, "autotune: no legal tiling");
    std::sort(timed.begin(), timed.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    // pass 2: the contenders within 8 % of the best are re-timed twice with 8 launches each (clocks are warm
    // by now and the order effect of pass 1 is gone); best of the three readings decides
    double best = timed[0].first;
    Variant bv = *timed[0].second;
    size_t ncont = 0;
    while (ncont < timed.size() && ncont < 4 && timed[ncont].first <= timed[0].first * 1.08) ++ncont;
    if (ncont > 1) {
        std::vector<double> score(ncont);
        for (size_t i = 0; i < ncont; ++i) score[i] = timed[i].first;
        for (int round = 0; round < 2; ++round)
            for (size_t i = 0; i < ncont; ++i) {
                double ms;
                if (int rc = time_variant(*timed[i].second, 8, ms)) return rc;
                score[i] = (round == 0) ? ms : std::min(score[i], ms); // pass-1 reading is replaced, not kept
            }
        size_t bi = 0;
        for (size_t i = 1; i < ncont; ++i)
            if (score[i] < score[bi]) bi = i;
        best = score[bi];
        bv = *timed[bi].second;
        if (verbose)
            for (size_t i = 0; i < ncont; ++i) fprintf(stderr, "[pp autotune] %-28s   retime %-26s %8.1f us\n", sig, timed[i].second->name, score[i] * 1e3);
    }
    L.var = bv;
    tune_cache()[sig] = bv.name;
    if (verbose) fprintf(stderr, "[pp autotune] %-28s -> %s (%.1f us)\n", sig, bv.name, best * 1e3);
    return 0;
}

// PP_FORCE_VARIANT (tests): pin a tiling by name substring; "a;b": a where `ok` has one, else b.  The first entry of `ok` that a name
// matches goes to `out`.
static bool forced_variant(const std::vector<Variant>& ok, Variant& out)
{
    const char* force = getenv("PP_FORCE_VARIANT");
    if (!force) return false;
    const std::string all(force);
    for (size_t p = 0; p <= all.size();) {
        const size_t e = std::min(all.find(';', p), all.size());
        const std::string one = all.substr(p, e - p);
        for (const Variant& v : ok)
            if (strstr(v.name, one.c_str())) { out = v; return true; }
        p = e + 1;
    }
    return false;
}

// The tiling of one layer: PP_FORCE_VARIANT, the tune cache, or (measure) the fastest legal entry of its menu on the device.
// `shape` carries the layer's maps and the tuner's tensors.
static int autotune_layer(pp_ctx* ctx, Layer& L, const ConvCall& shape, bool verbose, bool measure)
{
    pp_net* net = (pp_net*)ctx->net;
    const int eprec = net->eff_prec, rows = layer_rows(ctx, L);
    const bool head9 = ctx->cfg.num_anchor_per_loc == 9, roofline = L.kind == 0 && L.stride == 1 && L.level == 0;
    auto legal = [&](const Variant& v) { return tiling_legal(v, rows, L.cin, shape.Hin, shape.Win, shape.Wout); };
    std::vector<Variant> menu, ok;
    layer_menu(L.kind, L.stride, L.up, menu, L.cin, roofline, head9, eprec, L.kind == 0 && L.stride == 2 && L.level == 0);
    std::copy_if(menu.begin(), menu.end(), std::back_inserter(ok), legal);
    if (eprec && ok.empty()) {
        // a shape none of the reduced-precision tilings takes (odd maps, Cin not a multiple of 16 / 32) runs its fp32 tilings:
        // pp_layer_tilings reports what really runs
        menu.clear();
        layer_menu(L.kind, L.stride, L.up, menu, L.cin, roofline, head9, 0);
        std::copy_if(menu.begin(), menu.end(), std::back_inserter(ok), legal);
    }
    if (!measure) { // no on-device tuning (PP_AUTOTUNE=0 / maps the tuner's buffers do not fit): fp32 keeps pick_variant's choice,
                    // a reduced-precision mode takes the first legal entry of its menu
        if (eprec)
            for (const Variant& v : ok)
                if (v.prec == (eprec == 4 ? 3 : eprec)) { L.var = v; return 0; }
        return 0;
    }
    // the key carries the library version and the menu size (an entry of another build's menu is not trusted), not the
    // device index: the GPUs of a node are identical, and ranks must be able to share rank 0's table
    char sig[160];
    snprintf(sig, sizeof(sig), "v%d m%d k%d s%d u%d c%d r%d %dx%d n%d b%d p%d", pp_version(), (int)menu.size(), L.kind, L.stride, L.up, L.cin, L.cout,
             shape.Hout, shape.Wout, ctx->cfg.norm_kind, tune_frames(ctx), eprec);
    if (forced_variant(ok, L.var)) return 0;
    auto hit = tune_cache().find(sig);
    if (hit != tune_cache().end())
        for (const Variant& v : menu)
            if (hit->second == v.name) { L.var = v; return 0; }
    return time_layer(ctx, L, ok, sig, shape, verbose);
}

// Shapes of the cls-only pass, timed like a layer's tilings (3 launches after a warm-up, the fastest is kept and cached).
static int autotune_head_cls(pp_ctx* ctx, float* tin, bool verbose, bool measure)
{
    pp_net* net = (pp_net*)ctx->net;
    std::vector<Variant> menu;
    gemm1x1_cls_menu(menu);
    for (const Variant& v : menu)
        PP_HIP(hipFuncSetAttribute((const void*)v.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g1_lds(v, 320)));
    net->cls_var = menu[0];
    if (!measure) return 0;
    if (forced_variant(menu, net->cls_var)) return 0; // like a layer's tiling: before the cache and the timing
    const int tb = tune_frames(ctx);
    char sig[160];
    snprintf(sig, sizeof(sig), "v%d m%d headcls %s %dx%d n%d b%d", pp_version(), (int)menu.size(), net->layers.back().var.name, ctx->H, ctx->W, ctx->cfg.norm_kind, tb);
    auto hit = tune_cache().find(sig);
    if (hit != tune_cache().end())
        for (const Variant& v : menu)
            if (hit->second == v.name) { net->cls_var = v; return 0; }
    NormRef pre;
    pre.mode = PRE_AFFINE; pre.scale = net->ones; pre.shift = net->zeros;
    double best = 1e30;
    for (const Variant& v : menu) {
        double ms;
        if (int rc = time_launches(ctx, 3, [&] { return launch_head_cls(ctx, v, tin, pre, ctx->f_cls, tb, 0); }, ms)) return rc;
        if (verbose) fprintf(stderr, "[pp autotune] %-28s %-34s %8.1f us\n", sig, v.name, ms * 1e3);
        if (ms < best) { best = ms; net->cls_var = v; }
    }
    tune_cache()[sig] = net->cls_var.name;
    return 0;
}

} // namespace ppc

using namespace ppc;

// The tiling names of one menu, in menu order, one per line -- stateless and without a HIP call, so tests enumerate the menus on a
// machine without a device (include/pp_hip.h).
extern "C" int pp_menu_names(int which, int kind, int stride, int up, int cin, int prec, int head9, int first_conv, int rows, int Hin, int Win, int Wout,
                             char* buf, int cap)
{
    std::vector<Variant> menu;
    if (which == 0) {
        if (kind < 0 || kind > 2 || prec < 0 || prec > 4 || (kind == 0 && stride != 1 && stride != 2) || (kind == 1 && up != 1 && up != 2 && up != 4)) return -1;
        // (the level-0 twin of a Winograd tiling -- layer_menu's roofline_layer -- has the name, the shape and the rules of the plain one)
        layer_menu(kind, stride, up, menu, cin, false, head9 != 0, prec, first_conv != 0);
    } else if (which == 1) {
        gemm1x1_cls_menu(menu);
    } else if (which == 2) {
        for (Family f : {Family::Wino4, Family::Wino6}) { menu.push_back(strip_v(f)); menu.push_back(strip_h(f)); }
    } else
        return -1;
    std::string t;
    for (const Variant& v : menu)
        if (rows <= 0 || tiling_legal(v, rows, cin, Hin, Win, Wout)) t += std::string(v.name) + "\n";
    if (buf && cap > 0) {
        const size_t n = std::min((size_t)cap - 1, t.size());
        memcpy(buf, t.data(), n);
        buf[n] = 0;
    }
    return (int)t.size();
}

int pp_net_create(pp_ctx* ctx)
{
    pp_net* net = new pp_net();
    ctx->net = net;
    const int H = ctx->H, W = ctx->W;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, ctx->device) == hipSuccess && prop.multiProcessorCount > 0) net->num_cu = prop.multiProcessorCount;
        if (const char* e = getenv("PP_W4_STRIPS")) net->w4_strips = (e[0] == '0') ? 0 : (e[0] == '2') ? 2 : -1;
    }
    for (int l = 0; l < 3; ++l)
        for (int b = 0; b < 4; ++b)
        {   // W6_FRONT_PAD floats in front: wino6's dwordx4 patch pieces start one float before a row (row 0 of channel 0 of frame 0 included)
            PP_HIP(hipMalloc((void**)&net->buf[l][b], ((size_t)ctx->max_batch * kC[l] * ((H >> l) + 1) * ((W >> l) + 1) + W6_FRONT_PAD) * sizeof(float)));
            net->buf[l][b] += W6_FRONT_PAD;
        }
    PP_HIP(hipMalloc((void**)&net->up, (size_t)ctx->max_batch * 320 * H * W * sizeof(float)));
    // statistics accumulators: one slot of [NREP][256][2] doubles per normalisation site (<= 24 sites)
    net->stats_bytes = (size_t)ctx->max_batch * 24 * NREP * 320 * 2 * sizeof(double);
    PP_HIP(hipMalloc((void**)&net->stats, net->stats_bytes));
    PP_HIP(hipMalloc((void**)&net->aff, (size_t)ctx->max_batch * 640 * sizeof(float)));
    PP_HIP(hipMalloc((void**)&net->bn_scale, (size_t)24 * 320 * sizeof(float)));
    PP_HIP(hipMalloc((void**)&net->bn_shift, (size_t)24 * 320 * sizeof(float)));
    PP_HIP(hipMalloc((void**)&net->head_bias, (size_t)head_rows(ctx->cfg.num_anchor_per_loc) * sizeof(float)));
    PP_HIP(hipMalloc((void**)&net->head_bias_perm, 96 * sizeof(float)));
    PP_HIP(hipMalloc((void**)&net->ones, 320 * sizeof(float)));
    PP_HIP(hipMalloc((void**)&net->zeros, 320 * sizeof(float)));
    std::vector<float> one(320, 1.f);
    PP_HIP(hipMemcpy(net->ones, one.data(), 320 * sizeof(float), hipMemcpyHostToDevice));
    PP_HIP(hipMemset(net->zeros, 0, 320 * sizeof(float)));
    // layer list in execution order
    int cin = 64;
    for (int b = 0; b < 3; ++b) {
        const int c = kC[b];
        char key[128];
        snprintf(key, sizeof(key), "rpn.block%d.0.weight", b + 1);
        net->layers.push_back(Layer{key, 0, cin, c, 2, 1, b, pick_variant(0, 2, 1, c, H >> b, W >> b)});
        for (int u = 0; u < block_units(b); ++u) {
            snprintf(key, sizeof(key), "rpn.block%d.%d.conv_block.2.weight", b + 1, 3 + u);
            net->layers.push_back(Layer{key, 0, c, c, 1, 1, b, pick_variant(0, 1, 1, c, H >> b, W >> b)});
            if (unit_two_convs(b, u)) {
                snprintf(key, sizeof(key), "rpn.block%d.%d.conv_block.5.weight", b + 1, 3 + u);
                net->layers.push_back(Layer{key, 0, c, c, 1, 1, b, pick_variant(0, 1, 1, c, H >> b, W >> b)});
            }
        }
        const int up = 1 << b;
        snprintf(key, sizeof(key), "rpn.deconv%d.0.weight", b + 1);
        net->layers.push_back(Layer{key, 1, c, (b == 0) ? 64 : 128, 1, up, b, pick_variant(1, 1, up, ((b == 0) ? 64 : 128) * up * up, H >> b, W >> b)});
        cin = c;
    }
    net->layers.push_back(Layer{"heads", 2, 320, 10 * ctx->cfg.num_anchor_per_loc, 1, 1, 0,
                                pick_variant(2, 1, 1, head_rows(ctx->cfg.num_anchor_per_loc), H, W, ctx->cfg.num_anchor_per_loc == 9)});
    for (Layer& L : net->layers)
        PP_HIP(hipFuncSetAttribute((const void*)L.var.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.var.lds));
    for (Family f : {Family::Wino4, Family::Wino6})
        for (const Variant* sv : {&strip_v(f), &strip_h(f)})
            PP_HIP(hipFuncSetAttribute((const void*)sv->kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sv->lds));
    return 0;
}

void pp_net_destroy(pp_ctx* ctx)
{
    pp_net* net = (pp_net*)ctx->net;
    if (!net) return;
    for (int l = 0; l < 3; ++l)
        for (int b = 0; b < 4; ++b)
            if (net->buf[l][b]) (void)hipFree(net->buf[l][b] - W6_FRONT_PAD);
    for (Layer& L : net->layers)
        if (L.w) (void)hipFree(L.w);
    void* ptrs[] = {net->dbg_stats, net->up, net->stats, net->aff, net->bn_scale, net->bn_shift, net->bnp_scale, net->bnp_shift, net->head_bias, net->head_bias_perm, net->ones, net->zeros};
    for (void* q : ptrs)
        if (q) (void)hipFree(q);
    delete net;
    ctx->net = nullptr;
}

// BatchNorm2d(eval, eps 1e-3) of the _export/_trt nets folded to (scale, shift) for norm site `site`
// BatchNorm2d(eval, eps 1e-3) of the _export/_trt nets folded to (scale, shift) for channels [coff, coff + C) of norm site `site`
static int fold_bn(pp_ctx* ctx, const std::string& prefix, int C, int site, int coff = 0)
{
    pp_net* net = (pp_net*)ctx->net;
    auto get = [&](const char* s) -> const std::vector<float>* {
        auto it = ctx->host_w.find(prefix + s);
        if (it == ctx->host_w.end() || (int)it->second.data.size() != C) return nullptr;
        return &it->second.data;
    };
    const std::vector<float>*g = get(".weight"), *b = get(".bias"), *rm = get(".running_mean"), *rv = get(".running_var");
    if (!g || !b || !rm || !rv) return pp_fail(ctx, PP_E_NAME, ("missing BatchNorm tensors for " + prefix).c_str());
    std::vector<float> sc(C), sh(C);
    for (int c = 0; c < C; ++c) {
        double s = (double)(*g)[c] / std::sqrt((double)(*rv)[c] + 1e-3);
        sc[c] = (float)s;
        sh[c] = (float)((double)(*b)[c] - (double)(*rm)[c] * s);
    }
    PP_HIP(hipMemcpy(net->bn_scale + (size_t)site * 320 + coff, sc.data(), C * sizeof(float), hipMemcpyHostToDevice));
    PP_HIP(hipMemcpy(net->bn_shift + (size_t)site * 320 + coff, sh.data(), C * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// the nineteen BatchNorm2d layers of the RPN in state_dict order, each with its site
struct BnSite { std::string prefix; int C, site, coff; };
static std::vector<BnSite> bn_sites()
{
    std::vector<BnSite> out;
    for (int b = 0; b < 3; ++b) {
        char key[128];
        const int c = kC[b];
        snprintf(key, sizeof(key), "rpn.block%d.1", b + 1);
        out.push_back({key, c, site_block(b, 0), 0});
        for (int u = 0; u < block_units(b); ++u) {
            snprintf(key, sizeof(key), "rpn.block%d.%d.conv_block.0", b + 1, 3 + u);
            out.push_back({key, c, site_block(b, 1 + 2 * u), 0});
            if (unit_two_convs(b, u)) {
                snprintf(key, sizeof(key), "rpn.block%d.%d.conv_block.3", b + 1, 3 + u);
                out.push_back({key, c, site_block(b, 2 + 2 * u), 0});
            }
        }
        snprintf(key, sizeof(key), "rpn.deconv%d.1", b + 1);
        // deconv norms are stored contiguously at site 7 (block 0), channels [0,64),[64,192),[192,320)
        out.push_back({key, (b == 0) ? 64 : 128, 7, (b == 0) ? 0 : (b == 1 ? 64 : 192)});
    }
    return out;
}

// every BatchNorm of the RPN -> its site (the BatchNorm variant of the network)
static int fold_all_bn(pp_ctx* ctx)
{
    for (const BnSite& s : bn_sites())
        if (int rc = fold_bn(ctx, s.prefix, s.C, s.site, s.coff)) return rc;
    return 0;
}

// ---- the fold on the device: fold_bn's fp64 expression, each value rounded once, so the arrays equal those of a fresh commit of the
// same values bit for bit.  One workgroup per job (C <= 256) --------------------------------------------------------------------------
namespace {
constexpr int BN_LAYERS = 19;
struct BnFoldJob { const float *gamma, *beta, *rm, *rv; float *scale, *shift; int C; };
struct BnFoldJobs { BnFoldJob j[BN_LAYERS]; };

__global__ void __launch_bounds__(256) bn_fold_kernel(const BnFoldJobs jobs)
{
    const BnFoldJob& j = jobs.j[blockIdx.x];
    const int c = threadIdx.x;
    if (c >= j.C) return;
    const double s = (double)j.gamma[c] / sqrt((double)j.rv[c] + 1e-3);
    j.scale[c] = (float)s;
    j.shift[c] = (float)((double)j.beta[c] - (double)j.rm[c] * s);
}

// dgamma = r (dscale - running_mean dshift), dbeta = dshift with r = 1 / sqrt(running_var + 1e-3), in fp64, rounded once
__global__ void __launch_bounds__(256) bn_affine_grad_kernel(const double* __restrict__ dscale, const double* __restrict__ dshift,
                                                             const float* __restrict__ rm, const float* __restrict__ rv, float* __restrict__ dgamma,
                                                             float* __restrict__ dbeta, int C)
{
    const int c = threadIdx.x;
    if (c >= C) return;
    const double r = 1.0 / sqrt((double)rv[c] + 1e-3);
    dgamma[c] = (float)(r * (dscale[c] - (double)rm[c] * dshift[c]));
    dbeta[c] = (float)dshift[c];
}
} // namespace

extern "C" int pp_bn_fold(pp_ctx* ctx, int C, const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                          float* scale, float* shift, void* stream)
{
    if (!ctx) return PP_E_ARG;
    if (C < 1 || C > 256) return pp_fail(ctx, PP_E_ARG, "pp_bn_fold: C must be 1 .. 256");
    if (!gamma || !beta || !running_mean || !running_var || !scale || !shift) return pp_fail(ctx, PP_E_ARG, "pp_bn_fold: null pointer");
    if (((uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)running_mean | (uintptr_t)running_var | (uintptr_t)scale | (uintptr_t)shift) & 3)
        return pp_fail(ctx, PP_E_ARG, "pp_bn_fold: tensors must be 4-byte aligned");
    PP_HIP(hipSetDevice(ctx->device));
    BnFoldJobs jobs = {};
    jobs.j[0] = BnFoldJob{gamma, beta, running_mean, running_var, scale, shift, C};
    hipLaunchKernelGGL(bn_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, jobs);
    PP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pp_bn_affine_grad(pp_ctx* ctx, int C, const double* dscale, const double* dshift, const float* running_mean,
                                 const float* running_var, float* dgamma, float* dbeta, void* stream)
{
    if (!ctx) return PP_E_ARG;
    if (C < 1 || C > 256) return pp_fail(ctx, PP_E_ARG, "pp_bn_affine_grad: C must be 1 .. 256");
    if (!dscale || !dshift || !running_mean || !running_var || !dgamma || !dbeta) return pp_fail(ctx, PP_E_ARG, "pp_bn_affine_grad: null pointer");
    if ((((uintptr_t)dscale | (uintptr_t)dshift) & 7) || (((uintptr_t)running_mean | (uintptr_t)running_var | (uintptr_t)dgamma | (uintptr_t)dbeta) & 3))
        return pp_fail(ctx, PP_E_ARG, "pp_bn_affine_grad: misaligned tensor");
    PP_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(bn_affine_grad_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, dscale, dshift, running_mean, running_var, dgamma, dbeta, C);
    PP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pp_update_bn_fold(pp_ctx* ctx, const float* const* bn, void* stream)
{
    if (!ctx) return PP_E_ARG;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, "pp_update_bn_fold: weights not committed");
    if (ctx->cfg.norm_kind != 1) return pp_fail(ctx, PP_E_ARG, "pp_update_bn_fold: the BatchNorm backbone only (InstanceNorm has no affine to fold)");
    if (!bn) return pp_fail(ctx, PP_E_ARG, "pp_update_bn_fold: null pointer");
    for (int i = 0; i < 4 * BN_LAYERS; ++i)
        if (!bn[i] || ((uintptr_t)bn[i] & 3)) return pp_fail(ctx, PP_E_ARG, "pp_update_bn_fold: null or misaligned tensor pointer");
    pp_net* net = (pp_net*)ctx->net;
    PP_HIP(hipSetDevice(ctx->device));
    const std::vector<BnSite> sites = bn_sites();
    BnFoldJobs jobs = {};
    for (int i = 0; i < BN_LAYERS; ++i) {
        const size_t o = (size_t)sites[i].site * 320 + sites[i].coff;
        jobs.j[i] = BnFoldJob{bn[4 * i], bn[4 * i + 1], bn[4 * i + 2], bn[4 * i + 3], net->bn_scale + o, net->bn_shift + o, sites[i].C};
    }
    hipLaunchKernelGGL(bn_fold_kernel, dim3(BN_LAYERS), dim3(256), 0, (hipStream_t)stream, jobs);
    PP_HIP(hipGetLastError());
    return 0;
}

// the head's bias in natural row order and, for the 9-anchor head, in gemm1x1's
static int commit_head_bias(pp_ctx* ctx)
{
    pp_net* net = (pp_net*)ctx->net;
    const int na = ctx->cfg.num_anchor_per_loc;
    std::vector<float> hbv((size_t)head_rows(na), 0.f);
    float* hb = hbv.data();
    int r0 = 0;
    for (const HeadPart& part : kHead) {
        const int cnt = part.rows_per_anchor * na;
        auto w = ctx->host_w.find(part.bias);
        if (w == ctx->host_w.end() || (int)w->second.data.size() != cnt)
            return pp_fail(ctx, PP_E_NAME, (std::string("missing/mis-shaped ") + part.bias).c_str());
        memcpy(hb + r0, w->second.data.data(), sizeof(float) * cnt);
        r0 += cnt;
    }
    PP_HIP(hipMemcpy(net->head_bias, hb, hbv.size() * sizeof(float), hipMemcpyHostToDevice));
    if (na == 9) {
        float hp[96];
        for (int t = 0; t < 96; ++t) hp[t] = head_tile_row(t) >= 0 ? hb[head_tile_row(t)] : 0.f;
        PP_HIP(hipMemcpy(net->head_bias_perm, hp, sizeof(hp), hipMemcpyHostToDevice));
    }
    return 0;
}

namespace {
struct TuneBufs { // the tuner's input and output tensors, freed at scope exit
    float *in = nullptr, *out = nullptr;
    ~TuneBufs()
    {
        if (in) (void)hipFree(in - W6_FRONT_PAD);
        if (out) (void)hipFree(out);
    }
};
} // namespace

int pp_net_commit(pp_ctx* ctx)
{
    pp_net* net = (pp_net*)ctx->net;
    if (int rc = commit_head_bias(ctx)) return rc;
    const char* at = getenv("PP_AUTOTUNE");
    const char* vb = getenv("PP_VERBOSE");
    const bool tune = !(at && at[0] == '0');
    const bool verbose = vb && vb[0] != '0';
    const int H = ctx->H, W = ctx->W, na = ctx->cfg.num_anchor_per_loc;
    TuneBufs t;
    const bool can_tune = tune && (H % 4 == 0) && (W % 4 == 0);
    // fp16 storage of the activations needs every conv on conv16's and every upsampler / the head on gemm1x1's 16-bit-tensor
    // tilings: maps a multiple of 4 wide at all three levels and the 9-anchor head; otherwise mode 4 runs as mode 3 (fp32 tensors)
    net->up16 = ctx->precision == 4 && (W % 16 == 0) && ((H * W) % 64 == 0) && na == 9;
    net->eff_prec = (ctx->precision == 4 && !net->up16) ? 3 : ctx->precision;
    if (can_tune) {
        const size_t nin = std::max((size_t)64 * ctx->gx * ctx->gy, (size_t)320 * H * W);
        const int tb = tune_frames(ctx);
        PP_HIP(hipMalloc((void**)&t.in, ((size_t)tb * nin + 256 + W6_FRONT_PAD) * sizeof(float)));
        t.in += W6_FRONT_PAD;
        PP_HIP(hipMalloc((void**)&t.out, ((size_t)tb * 320 * H * W + 256) * sizeof(float)));
        hipLaunchKernelGGL(fill_pattern, dim3(2048), dim3(256), 0, 0, t.in, (size_t)tb * nin);
    }
    for (Layer& L : net->layers) {
        ConvCall shape; // the layer's maps, on the tuner's tensors
        shape.in = t.in; shape.out = t.out;
        shape.Hout = H >> L.level; shape.Wout = W >> L.level;
        const int s = (L.kind == 0 && L.stride == 2) ? 2 : 1;
        shape.Hin = shape.Hout * s; shape.Win = shape.Wout * s;
        if (!can_tune && net->eff_prec == 0) L.var = pick_variant(L.kind, L.stride, L.up, layer_rows(ctx, L), shape.Hout, shape.Wout, na == 9);
        if (int rc = autotune_layer(ctx, L, shape, verbose, can_tune)) return rc;
        PP_HIP(hipFuncSetAttribute((const void*)L.var.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)layer_lds(L.var, L.cin)));
        if (L.var.kern2) PP_HIP(hipFuncSetAttribute((const void*)L.var.kern2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.var.lds));
        if (int rc = pack_layer(ctx, L)) return rc;
    }
    ctx->sc1_kc = (net->layers[0].var.family == Family::Direct && net->layers[0].var.kc == 8) ? 8 : 4;
    // deferred head: fp32 plan with the 9-anchor head on a gemm1x1 tiling (its image is what the cls pass and the candidate head read)
    const Layer& head = net->layers.back();
    net->defer_ok = net->eff_prec == 0 && na == 9 && head.var.family == Family::Gemm1x1 && head.var.prec == 0 && head.var.io16 == 0;
    if (net->defer_ok)
        if (int rc = autotune_head_cls(ctx, t.in, verbose, can_tune)) return rc;
    if (t.in) { // the tuner's launches are done before its tensors go
        PP_HIP(hipDeviceSynchronize());
        tune_cache_save();
    }
    if (net->up16)
        for (const Layer& L : net->layers)
            if ((L.kind == 1 && L.var.io16 != 3) || (L.kind == 2 && L.var.io16 != 1) ||
                (L.kind == 0 && L.var.io16 != ((L.stride == 2 && L.level == 0) ? 2 : 3)))
                return pp_fail(ctx, PP_E_STATE, "fp16s: a layer did not get a 16-bit-tensor tiling (PP_FORCE_VARIANT?)");
    return ctx->cfg.norm_kind == 1 ? fold_all_bn(ctx) : 0;
}
