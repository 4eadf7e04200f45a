// What conv_igemm.hip decides for some fifty hand-written descriptors, printed without a GPU: the five routing queries' answers,
// abc_conv_fwd's status with its error text and the launch it makes -- for the general kernel the grid, the dynamic LDS size and every
// field of the argument block (pointers as null / non-null), for the other families the family and, for the lean kernel, the geometry
// the route hands over -- and abc_conv_batch_ok / abc_conv_fwd_batch for two arrays.  Built twice, with -ftrivial-auto-var-init=zero and
// =pattern on the host side, the two outputs are identical exactly when no decision reads an uninitialised local; run on two revisions
// of conv_igemm.hip, they are identical exactly when both decide, refuse and launch alike.
//
//   cd abc-net_amd/csrc
//   for v in zero pattern; do
//     hipcc --offload-arch=gfx950 --cuda-host-only -O3 -std=c++17 -Xarch_host -ftrivial-auto-var-init=$v -I. -x hip -c ../../profiles/tools/conv_route_dump.cpp -o /tmp/cd_$v.o
//     hipcc --cuda-host-only /tmp/cd_$v.o -Wl,--defsym=$(nm /tmp/cd_$v.o | grep -o '__hip_fatbin_[0-9a-f]*' | head -1)=0 -L.. -labcnet_hip -Wl,-rpath,$PWD/.. -o /tmp/cd_$v
//     /tmp/cd_$v > /tmp/cd_$v.txt
//   done; cmp /tmp/cd_zero.txt /tmp/cd_pattern.txt
//
// The host side alone is compiled (the device image's symbol is defined as absent).  conv_igemm.hip is included whole and its launches
// are caught by the macro below; the other families' launch functions are replaced by the ones at the end of this file, their `ok`
// functions, abc_conv_fast_geom and abc_fail come from the library.  The program knows none of conv_igemm.hip's internals and runs
// against any revision of it.
#include "common.hpp"
#include "capi_util.hpp"
#include "conv_fast.hpp"
#include <stdio.h>
#include <string.h>

template <class K>
static auto dump_args(const K& k, int) -> decltype((void)k.nblocks_n) {
    printf("    src: x=%d scale=%d shift=%d slope=%d Hx=%d Wx=%d ldx=%d pool=%d drop_p=%g drop_seed=%u planar=%d ctot=%d drop_salt=%d\n", k.src.x != nullptr,
           k.src.scale != nullptr, k.src.shift != nullptr, k.src.slope != nullptr, k.src.Hx, k.src.Wx, k.src.ldx, k.src.pool, (double)k.src.drop_p, k.src.drop_seed,
           k.src.planar, k.src.ctot, k.src.drop_salt != nullptr);
    printf("    w=%d bias=%d y=%d stats=%d B=%d Hin=%d Win=%d cin_off=%d Cin=%d nchunks=%d Hg=%d Wg=%d Hout=%d Wout=%d ldy=%d cout_off=%d Cout=%d Cout_pad=%d\n",
           k.w != nullptr, k.bias != nullptr, k.y != nullptr, k.stats != nullptr, k.B, k.Hin, k.Win, k.cin_off, k.Cin, k.nchunks, k.Hg, k.Wg, k.Hout, k.Wout, k.ldy,
           k.cout_off, k.Cout, k.Cout_pad);
    printf("    om=%d oy0=%d ox0=%d ntaps=%d tg=%d ngroups=%d dy_min=%d dx_min=%d HH=%d HW=%d RS=%d tiles=%dx%d nblocks_n=%d sA_bytes=%d a_bufs=%d sB_off=%d sB_bytes=%d\n",
           k.om, k.oy0, k.ox0, k.ntaps, k.tg, k.ngroups, k.dy_min, k.dx_min, k.HH, k.HW, k.RS, k.tiles_x, k.tiles_y, k.nblocks_n, k.sA_bytes, k.a_bufs, k.sB_off, k.sB_bytes);
    printf("    tap_off=%d coef_off=%d cstride=%d planar_out=%d ctot_out=%d fast_a=%d ntiles=%d b_static=%d stg_off=%d stats_rows=%d accumulate=%d magic=%d out_act=%d "
           "out_slope=%g bytesA=%u bytesW=%u\n", k.tap_off, k.coef_off, k.cstride, k.planar_out, k.ctot_out, k.fast_a, k.ntiles, k.b_static, k.stg_off, k.stats_rows,
           k.accumulate, k.magic, k.out_act, (double)k.out_slope, k.bytesA, k.bytesW);
    printf("    taps:");
    for (int t = 0; t < k.ntaps; ++t) printf(" (%d,%d)", k.ty[t], k.tx[t]);
    printf("\n");
}
template <class K>
static void dump_args(const K&, long) {}

template <class K>
static void dump_launch(const char* fn, dim3 grid, dim3 block, int lds, const K& k) {
    // (the kernel's name as the source spells it: `fn` for an instantiation picked through a pointer)
    printf("  launch %s grid=(%u,%u,%u) block=%u lds=%d\n", fn, grid.x, grid.y, grid.z, block.x, lds);
    dump_args(k, 0);
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(fn, grid, block, lds, st, ...) dump_launch(#fn, grid, block, lds, __VA_ARGS__)

// (no device here: a launch always "succeeds")
int abc_allow_lds(const void*, int, unsigned long long*) { return 0; }
int abc_check_launch(const char*) { return 0; }

#include "conv_igemm.hip"

static char* const some = (char*)0x1000;

// k x k, stride 1, "same" size: the producer's BatchNorm + activation on load, bias, no statistics
static abc_conv_desc conv(int dt, int B, int H, int W, int Cin, int Cout, int k) {
    abc_conv_desc d;
    memset(&d, 0, sizeof d);
    d.src.x = some; d.src.scale = (const float*)some; d.src.shift = (const float*)some; d.src.slope = (const float*)some;
    d.src.Hx = H; d.src.Wx = W; d.src.ldx = Cin;
    d.w = some; d.bias = (const float*)some; d.y = some;
    d.dtype_in = d.dtype_c = d.dtype_out = dt;
    d.B = B; d.Hin = d.Hg = d.Hout = H; d.Win = d.Wg = d.Wout = W; d.Cin = Cin; d.ldy = d.Cout = Cout; d.Cout_pad = (Cout + 31) / 32 * 32;
    d.stride = 1; d.om = 1; d.stats_rows = 2;
    d.ntaps = k * k;
    for (int t = 0; t < k * k; ++t) { d.tap_dy[t] = (int8_t)(t / k - k / 2); d.tap_dx[t] = (int8_t)(t % k - k / 2); }
    return d;
}

static abc_conv_desc with_stats(abc_conv_desc d) { d.stats = (float*)some; return d; }

// act_bwd in the epilogue of a data gradient: no transform on load, no bias, the producer's raw output and its five coefficient rows
static abc_conv_desc actbwd(abc_conv_desc d) {
    d.src.scale = d.src.shift = d.src.slope = nullptr; d.bias = nullptr;
    d.actbwd_y = some; d.actbwd_ld = d.Cout;
    d.actbwd_scale = d.actbwd_shift = d.actbwd_slope = d.actbwd_mean = d.actbwd_invstd = (const float*)some;
    return with_stats(d);
}

// the folded inference graph's 3x3 over finished features
static abc_conv_desc folded(abc_conv_desc d) {
    d.src.scale = d.src.shift = d.src.slope = nullptr;
    d.out_act = 1; d.out_slope = 0.01f;
    return d;
}

static abc_conv_desc fp8(abc_conv_desc d) {
    d = folded(d);
    d.dtype_in = d.dtype_c = d.dtype_out = ABC_FP8;
    d.out_scale = (const float*)some; d.out_quant = (const float*)some;
    return d;
}

static abc_conv_desc head_fwd(int dt_c) {
    abc_conv_desc d = conv(dt_c, 16, 96, 96, 128, 14, 1);
    d.dtype_in = dt_c; d.dtype_out = ABC_F32; d.planar_out = 1; d.ctot_out = 14; d.ldy = 0;
    return d;
}

static void show(const char* what, const abc_conv_desc& d) {
    int32_t bn = -7, mt = -7, ck = -7;
    const int rt = abc_conv_tile(&d, &bn, &mt, &ck);
    printf("%s\n  variant=%d weight_layout=%d stat_blocks=%d tile=(%d: %d, %d, %d) actbwd_ok=%d\n", what, abc_conv_variant(&d), abc_conv_weight_layout(&d),
           abc_conv_stat_blocks(&d), rt, bn, mt, ck, abc_conv_actbwd_ok(&d));
    const int rc = abc_conv_fwd(&d, nullptr);
    if (rc) printf("  abc_conv_fwd=%d \"%s\"\n", rc, abc_last_error());
    else printf("  abc_conv_fwd=0\n");
}

template <class F>
static void show(const char* what, abc_conv_desc d, F change) { change(d); show(what, d); }

int main() {
    const abc_conv_desc trunk = conv(ABC_BF16, 16, 96, 96, 128, 128, 3), deep = conv(ABC_BF16, 2, 24, 24, 64, 64, 3), n16 = conv(ABC_BF16, 16, 384, 384, 16, 16, 3);
    // ---- one per family
    show("general: pooled input, 64 -> 64 3x3 at 24 x 24 from 48 x 48, bf16, statistics", with_stats(deep), [](abc_conv_desc& d) { d.src.Hx = d.src.Wx = 48; d.src.pool = 1; });
    show("general: dropout on load, 128 -> 128 3x3 at 96 x 96, bf16, four statistics rows", with_stats(trunk), [](abc_conv_desc& d) { d.src.drop_p = 0.2f; d.src.drop_seed = 7; d.stats_rows = 4; });
    show("general: ragged 40 -> 24 channels at 72 x 88, f32", conv(ABC_F32, 1, 72, 88, 40, 24, 3));
    show("general: stride 2, f32 in, bf16 out, 5x5 taps", conv(ABC_BF16, 2, 48, 48, 40, 64, 5), [](abc_conv_desc& d) { d.dtype_in = ABC_F32; d.stride = 2; d.Hg = d.Hout = d.Wg = d.Wout = 24; });
    show("lean, weights-direct: trunk 128 -> 128 3x3 at 96 x 96, bf16, statistics", with_stats(trunk));
    show("lean, weights-direct: the same without statistics", trunk);
    show("lean, staged weights: 64 -> 32 3x3 at 24 x 24, bf16, statistics", with_stats(conv(ABC_BF16, 2, 24, 24, 64, 32, 3)));
    show("lean: 64 -> 64 3x3 at 24 x 24, f32", conv(ABC_F32, 2, 24, 24, 64, 64, 3));
    show("stem: 1 -> 16 3x3 at 384 x 384, f32 image, bf16 out, statistics", with_stats(conv(ABC_BF16, 16, 384, 384, 1, 16, 3)),
         [](abc_conv_desc& d) { d.dtype_in = ABC_F32; d.src.scale = d.src.shift = d.src.slope = nullptr; });
    show("head_fwd: 128 -> 14 1x1 at 96 x 96 into NCHW f32", head_fwd(ABC_BF16));
    show("head_fwd with the NMS output", head_fwd(ABC_BF16), [](abc_conv_desc& d) { d.head_aux = (float*)some; d.head_aux_mode = 1; });
    show("head_dgrad: 14 planar f32 -> 128 1x1 at 96 x 96", conv(ABC_BF16, 16, 96, 96, 14, 128, 1), [](abc_conv_desc& d) {
        d.dtype_in = ABC_F32; d.src.planar = 1; d.src.ctot = 14; d.src.ldx = 0; d.src.scale = d.src.shift = d.src.slope = nullptr; d.bias = nullptr; });
    show("narrow: 16 -> 16 3x3 at 384 x 384, bf16, statistics", with_stats(n16));
    show("narrow: 32 -> 32 5x5 at 96 x 96 (unet2), four statistics rows", with_stats(conv(ABC_BF16, 4, 96, 96, 32, 32, 5)), [](abc_conv_desc& d) { d.stats_rows = 4; });
    show("narrow with the pooled copy", with_stats(n16), [](abc_conv_desc& d) { d.pool_y = some; d.ld_pool = 16; });
    // ---- act_bwd in the epilogue: both servers, and refused
    show("act_bwd by the lean kernel: trunk data gradient", actbwd(trunk));
    show("act_bwd by the narrow-level kernel: 16 -> 16", actbwd(n16));
    show("act_bwd asked with `stats` still NULL", actbwd(trunk), [](abc_conv_desc& d) { d.stats = nullptr; });
    show("act_bwd refused: f32", actbwd(conv(ABC_F32, 2, 24, 24, 64, 64, 3)));
    show("act_bwd refused: rows that are no whole tile (100 x 96)", actbwd(conv(ABC_BF16, 2, 100, 96, 128, 128, 3)), [](abc_conv_desc& d) { d.Wg = d.Wout = d.Win = d.src.Wx = 104; });
    show("act_bwd by the narrow-level kernel: 32 -> 32 3x3", actbwd(conv(ABC_BF16, 16, 384, 384, 32, 32, 3)));
    show("act_bwd refused: a narrow-level layer in a form that kernel does not fuse (with the pooled copy)", actbwd(n16), [](abc_conv_desc& d) { d.pool_y = some; d.ld_pool = 16; });
    show("act_bwd refused: the heads' 1x1 forward", head_fwd(ABC_BF16), [](abc_conv_desc& d) { d.actbwd_y = some; });
    show("act_bwd and heads_epi together", actbwd(trunk), [](abc_conv_desc& d) { d.heads_epi = (const abc_heads_epi*)some; });
    // ---- the heads' epilogue
    show("heads_epi: 128 -> 1024 3x3 at 96 x 96 over finished features", folded(conv(ABC_BF16, 16, 96, 96, 128, 1024, 3)), [](abc_conv_desc& d) { d.heads_epi = (const abc_heads_epi*)some; });
    show("heads_epi refused: no epilogue activation", folded(conv(ABC_BF16, 16, 96, 96, 128, 1024, 3)), [](abc_conv_desc& d) { d.heads_epi = (const abc_heads_epi*)some; d.out_act = 0; });
    // ---- fp8
    show("fp8: 128 -> 128 3x3 at 96 x 96", fp8(trunk));
    show("fp8 heads_epi", fp8(conv(ABC_BF16, 16, 96, 96, 128, 1024, 3)), [](abc_conv_desc& d) { d.heads_epi = (const abc_heads_epi*)some; });
    show("fp8 head_fwd", head_fwd(ABC_FP8), [](abc_conv_desc& d) { d.src.scale = d.src.shift = d.src.slope = nullptr; d.out_scale = (const float*)some; });
    show("fp8 refused: pooled input", fp8(trunk), [](abc_conv_desc& d) { d.src.pool = 1; });
    show("fp8 refused: alignment", fp8(trunk), [](abc_conv_desc& d) { d.cout_off = 8; d.ldy = 136; });
    show("fp8 refused: grid exceeds the output", fp8(trunk), [](abc_conv_desc& d) { d.Hout = 95; });
    show("fp8 refused: heads_epi into bf16", fp8(conv(ABC_BF16, 16, 96, 96, 128, 1024, 3)), [](abc_conv_desc& d) { d.heads_epi = (const abc_heads_epi*)some; d.dtype_out = ABC_BF16; });
    show("fp8 refused: 1x1", fp8(conv(ABC_BF16, 16, 96, 96, 128, 128, 1)));
    show("fp8 refused: 50 taps", fp8(trunk), [](abc_conv_desc& d) { d.ntaps = 50; });
    // ---- every other refusal of abc_conv_fwd, in its order
    show("refused: no taps", trunk, [](abc_conv_desc& d) { d.ntaps = 0; });
    show("refused: 50 taps", trunk, [](abc_conv_desc& d) { d.ntaps = 50; });
    show("refused: stride 3", trunk, [](abc_conv_desc& d) { d.stride = 3; });
    show("refused: no input channels", trunk, [](abc_conv_desc& d) { d.Cin = 0; });
    show("refused: Cout_pad", trunk, [](abc_conv_desc& d) { d.Cout_pad = 120; });
    show("refused: taps too far apart for the LDS", with_stats(deep), [](abc_conv_desc& d) { d.src.Hx = d.src.Wx = 48; d.src.pool = 1; d.tap_dy[0] = -100; d.tap_dx[0] = -100; d.tap_dy[8] = 100; d.tap_dx[8] = 100; });
    show("refused: pooled dims", deep, [](abc_conv_desc& d) { d.src.pool = 1; });
    show("refused: dims", deep, [](abc_conv_desc& d) { d.src.Hx = 25; });
    show("refused: input alignment", deep, [](abc_conv_desc& d) { d.cin_off = 4; d.src.ldx = 68; });
    show("refused: planar bf16 input", deep, [](abc_conv_desc& d) { d.src.planar = 1; d.src.ctot = 64; });
    show("refused: planar bf16 output", deep, [](abc_conv_desc& d) { d.planar_out = 1; d.ctot_out = 64; });
    show("refused: planar output with an activation", conv(ABC_F32, 2, 24, 24, 64, 64, 3), [](abc_conv_desc& d) { d.planar_out = 1; d.ctot_out = 64; d.out_act = 1; });
    show("refused: accumulate into a planar output", conv(ABC_F32, 2, 24, 24, 64, 64, 3), [](abc_conv_desc& d) { d.planar_out = 1; d.ctot_out = 64; d.accumulate = 1; });
    show("refused: grid exceeds the output", deep, [](abc_conv_desc& d) { d.om = 2; });
    show("refused: stem_x outside the narrow-level kernel", deep, [](abc_conv_desc& d) { d.stem_x = (const float*)some; });
    show("refused: pool_y outside the narrow-level kernel", trunk, [](abc_conv_desc& d) { d.pool_y = some; });
    show("refused: head_aux outside the heads' kernel", trunk, [](abc_conv_desc& d) { d.head_aux = (float*)some; d.head_aux_mode = 1; });
    show("refused: f32 compute from bf16", conv(ABC_F32, 1, 72, 88, 40, 24, 3), [](abc_conv_desc& d) { d.dtype_in = ABC_BF16; });
    show("refused: f32 in and out around bf16 compute", conv(ABC_BF16, 1, 72, 88, 40, 24, 3), [](abc_conv_desc& d) { d.dtype_in = d.dtype_out = ABC_F32; });
    // ---- batches: the four output-parity phases of a ConvTranspose2d(128 -> 64, 3, stride 2) forward at 48 x 48, and two trunk layers
    {
        abc_conv_desc ph[4];
        const int nt[4] = {1, 2, 2, 4};
        for (int p = 0; p < 4; ++p) {
            ph[p] = conv(ABC_BF16, 16, 48, 48, 128, 64, 1);
            ph[p].Hout = ph[p].Wout = 96; ph[p].om = 2; ph[p].oy0 = p / 2; ph[p].ox0 = p % 2; ph[p].ntaps = nt[p];
            for (int t = 0; t < nt[p]; ++t) { ph[p].tap_dy[t] = (int8_t)((p / 2) ? t / (nt[p] / 2) : 0); ph[p].tap_dx[t] = (int8_t)((p % 2) ? t % 2 : 0); }
        }
        printf("batch: four phases of a transposed convolution\n  batch_ok=%d\n", abc_conv_batch_ok(ph, 4));
        printf("  abc_conv_fwd_batch=%d\n", abc_conv_fwd_batch(ph, 4, nullptr));
        abc_conv_desc two[2] = {trunk, with_stats(trunk)};
        printf("batch: two trunk layers, one with statistics\n  batch_ok=%d\n", abc_conv_batch_ok(two, 2));
        printf("  abc_conv_fwd_batch=%d\n", abc_conv_fwd_batch(two, 2, nullptr));
    }
    return 0;
}

// ---- the other families' launches: what the route chose and, for the lean kernel, the geometry it handed over
int abc_conv_stem_launch(const abc_conv_desc*, abc_stream_t) { printf("  launch stem.hip\n"); return 0; }
int abc_head_fwd_launch(const abc_conv_desc*, abc_stream_t) { printf("  launch heads.hip forward\n"); return 0; }
int abc_head_dgrad_launch(const abc_conv_desc*, abc_stream_t) { printf("  launch heads.hip data gradient\n"); return 0; }
int abc_conv_narrow_launch(const abc_conv_desc*, abc_stream_t) { printf("  launch conv_narrow.hip\n"); return 0; }
int abc_conv_fast_launch_batch(const abc_conv_desc*, int n, abc_stream_t) { printf("  launch conv_fast.hip, batch of %d\n", n); return 0; }
int abc_conv_fast_launch(const abc_conv_desc*, const abc_fast_geom& g, abc_stream_t) {
    printf("  launch conv_fast.hip eligible=%d CK=%d BN=%d MT=%d dy_min=%d dx_min=%d HH=%d HW=%d PS=%d RS=%d tg=%d ngroups=%d sA_bytes=%d a_bufs=%d sB_bytes=%d tap_off=%d\n"
           "    coef_off=%d cstride=%d lds=%d tiles=%dx%d nbn=%d ntiles=%d nwg=%d b_static=%d stg_off=%d red_off=%d wd=%d ystg_off=%d epi_off=%d m16=%d\n",
           g.eligible, g.CK, g.BN, g.MT, g.dy_min, g.dx_min, g.HH, g.HW, g.PS, g.RS, g.tg, g.ngroups, g.sA_bytes, g.a_bufs, g.sB_bytes, g.tap_off, g.coef_off, g.cstride,
           g.lds, g.tiles_x, g.tiles_y, g.nbn, g.ntiles, g.nwg, g.b_static, g.stg_off, g.red_off, g.wd, g.ystg_off, g.epi_off, g.m16);
    return 0;
}
