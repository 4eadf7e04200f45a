// What abc_wgrad decides for a dozen descriptors, printed without a GPU: the five routing queries' answers and, for the launches of the
// general kernel, the grid, the dynamic LDS size and every field of the argument block (pointers as null / non-null).  Built twice, with
// -ftrivial-auto-var-init=zero and =pattern on the host side, the two outputs are identical exactly when no decision reads an
// uninitialised local.
//
//   cd abc-net_amd/csrc
//   for v in zero pattern; do
//     hipcc --offload-arch=gfx950 --cuda-host-only -O3 -std=c++17 -Xarch_host -ftrivial-auto-var-init=$v -I. -x hip -c ../../profiles/tools/wgrad_route_dump.cpp -o /tmp/rd_$v.o
//     hipcc --cuda-host-only /tmp/rd_$v.o -Wl,--defsym=$(nm /tmp/rd_$v.o | grep -o '__hip_fatbin_[0-9a-f]*' | head -1)=0 -L.. -labcnet_hip -Wl,-rpath,$PWD/.. -o /tmp/rd_$v
//     /tmp/rd_$v > /tmp/rd_$v.txt
//   done; cmp /tmp/rd_zero.txt /tmp/rd_pattern.txt
//
// The host side alone is compiled (the device image's symbol is defined as absent); the other families' `ok` functions and abc_fail come from
// the library.  wgrad.hip is included whole and its launches are caught by the macro below, so the program knows none of its internals
// and runs against any revision of it.
#include "common.hpp"
#include "capi_util.hpp"
#include <stdio.h>
#include <string.h>

template <class K>
static auto dump_args(const K& k, int) -> decltype((void)k.qtab_off) {
    printf("    p: x=%d scale=%d Hx=%d Wx=%d ldx=%d pool=%d planar=%d ctot=%d drop_p=%g | q: x=%d scale=%d Hx=%d Wx=%d ldx=%d pool=%d planar=%d ctot=%d drop_p=%g\n",
           k.p.x != nullptr, k.p.scale != nullptr, k.p.Hx, k.p.Wx, k.p.ldx, k.p.pool, k.p.planar, k.p.ctot, (double)k.p.drop_p,
           k.q.x != nullptr, k.q.scale != nullptr, k.q.Hx, k.q.Wx, k.q.ldx, k.q.pool, k.q.planar, k.q.ctot, (double)k.q.drop_p);
    printf("    B=%d Hg=%d Wg=%d Hq=%d Wq=%d cp_off=%d Ca=%d cq_off=%d Cb=%d Ca_pad=%d Cb_pad=%d ntaps=%d tgw=%d nsplit=%d npatch=%d tiles=%dx%d\n",
           k.B, k.Hg, k.Wg, k.Hq, k.Wq, k.cp_off, k.Ca, k.cq_off, k.Cb, k.Ca_pad, k.Cb_pad, k.ntaps, k.tgw, k.nsplit, k.npatch, k.tiles_x, k.tiles_y);
    printf("    dy_min=%d dx_min=%d HH=%d HW=%d PSWP=%d PSWQ=%d sP=%d sQ=%d coef_off=%d cstrP=%d cstrQ=%d nta=%d ntb=%d fast=%d%d nbuf=%d\n",
           k.dy_min, k.dx_min, k.HH, k.HW, k.PSWP, k.PSWQ, k.sP_bytes, k.sQ_bytes, k.coef_off, k.cstrP, k.cstrQ, k.nta, k.ntb, k.fast_p, k.fast_q, k.nbuf);
    printf("    bytesP2=%u magicQ=%d k3=%d mg_tx=%u mg_ty=%u regP=%d qtab_off=%d bytesP=%u bytesQ=%u p2=%d p_out=%d ld_p2=%d cp2_off=%d ld_pout=%d\n",
           k.bytesP2, k.magicQ, k.k3, k.mg_tx, k.mg_ty, k.regP, k.qtab_off, k.bytesP, k.bytesQ, k.p2 != nullptr, k.p_out != nullptr, k.ld_p2, k.cp2_off, k.ld_pout);
    printf("    taps:");
    for (int t = 0; t < k.ntaps; ++t) printf(" (%d,%d)", k.ty[t], k.tx[t]);
    printf("\n");
}
template <class K>
static void dump_args(const K&, long) {}

template <class K, class... More>
static void dump_launch(const char* fn, dim3 grid, dim3 block, int lds, const K& k, const More&...) {
    // (the kernel's name as the source spells it: `fn` for an instantiation picked through a pointer)
    printf("  launch %s grid=(%u,%u,%u) block=%u lds=%d\n", fn, grid.x, grid.y, grid.z, block.x, lds);
    dump_args(k, 0);
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(fn, grid, block, lds, st, ...) dump_launch(#fn, grid, block, lds, __VA_ARGS__)

// (no device here: a launch always "succeeds")
int abc_allow_lds(const void*, int, unsigned long long*) { return 0; }
int abc_check_launch(const char*) { return 0; }

#include "wgrad.hip"

static abc_wgrad_desc conv(int dt, int B, int H, int W, int Ca, int Cb, int k) {
    abc_wgrad_desc d;
    memset(&d, 0, sizeof d);
    char* const some = (char*)0x1000;
    d.p.x = some; d.p.Hx = H; d.p.Wx = W; d.p.ldx = Ca;
    d.q.x = some; d.q.Hx = H; d.q.Wx = W; d.q.ldx = Cb;
    d.q.scale = (const float*)some; d.q.shift = (const float*)some; d.q.slope = (const float*)some;
    d.partial = (float*)some;
    d.dtype_p = d.dtype_q = d.dtype_c = dt;
    d.B = B; d.Hg = H; d.Wg = W; d.Hq = H; d.Wq = W; d.Ca = Ca; d.Cb = Cb; d.stride = 1; d.nsplit = 4;
    d.ntaps = k * k;
    for (int t = 0; t < k * k; ++t) { d.tap_dy[t] = (int8_t)(t / k - k / 2); d.tap_dx[t] = (int8_t)(t % k - k / 2); }
    return d;
}

static abc_wgrad_desc dual(abc_wgrad_desc d) {
    char* const some = (char*)0x1000;
    d.p.scale = (const float*)some; d.p.shift = (const float*)some; d.p.slope = (const float*)some;
    d.p2 = some; d.ld_p2 = d.Ca; d.cp2_off = 0; d.p_dual = 1; d.p_out = some; d.ld_pout = d.Ca;
    return d;
}

static void show(const char* what, const abc_wgrad_desc& d) {
    int32_t ca = -7, cb = -7, at = -7, bt = -7;
    const int rp = abc_wgrad_pads(&d, &ca, &cb), rt = abc_wgrad_tile(&d, &at, &bt);
    printf("%s\n  rowsum_ok=%d fuses_apply=%d pads=(%d: %d, %d) tile=(%d: %d, %d) blocks=%d\n", what, abc_wgrad_rowsum_ok(&d), abc_wgrad_fuses_apply(&d),
           rp, ca, cb, rt, at, bt, abc_wgrad_blocks(&d));
    // (the other families launch from their own files, not through the macro above)
    if (rt == 0 && at > 0) printf("  abc_wgrad=%d\n", abc_wgrad(&d, nullptr));
}

int main() {
    show("trunk 128 x 128 3x3 at 96 x 96, b16, with the correction on load", dual(conv(ABC_BF16, 16, 96, 96, 128, 128, 3)));
    show("trunk 128 x 128 3x3 at 96 x 96, b16, plain", conv(ABC_BF16, 16, 96, 96, 128, 128, 3));
    show("merged heads 1024 x 128 3x3 at 96 x 96, b16, with the correction on load", dual(conv(ABC_BF16, 16, 96, 96, 1024, 128, 3)));
    show("64 x 64 3x3 at 24 x 24, b16", conv(ABC_BF16, 16, 24, 24, 64, 64, 3));
    show("512 x 256 3x3 at 64 x 192, b1 (4 x 2 pairs)", conv(ABC_BF16, 1, 64, 192, 512, 256, 3));
    {
        // ConvTranspose2d(128 -> 64, 3, stride 2): P the 48 x 48 input, Q the gradient on the 96 x 96 grid inside a 128-wide buffer
        abc_wgrad_desc d = conv(ABC_BF16, 16, 48, 48, 128, 64, 3);
        d.q.scale = d.q.shift = d.q.slope = nullptr;
        d.q.Hx = d.q.Wx = d.Hq = d.Wq = 96; d.q.ldx = 128; d.cq_off = 64; d.stride = 2;
        for (int t = 0; t < 9; ++t) { d.tap_dy[t] = (int8_t)(t / 3); d.tap_dx[t] = (int8_t)(t % 3); }
        show("stride-2 transposed 128 x 64 at 48 x 48", d);
    }
    show("5x5 32 x 32 at 384 x 384 (unet2)", conv(ABC_BF16, 16, 384, 384, 32, 32, 5));
    show("5x5 64 x 32 at 96 x 96 (tap split)", conv(ABC_BF16, 4, 96, 96, 64, 32, 5));
    show("f32 64 x 32 3x3 at 64 x 64", conv(ABC_F32, 2, 64, 64, 64, 32, 3));
    show("ragged: 72 x 88, 40 x 24 channels, bf16", conv(ABC_BF16, 1, 72, 88, 40, 24, 3));
    {
        abc_wgrad_desc d = conv(ABC_BF16, 2, 24, 40, 64, 32, 3);
        d.q.Hx = 48; d.q.Wx = 80; d.q.pool = 1;
        show("pooled Q (general loader) 64 x 32 at 24 x 40", d);
    }
    show("16 x 16 3x3 at 384 x 384 (wgrad_narrow.hip)", conv(ABC_BF16, 16, 384, 384, 16, 16, 3));
    {
        abc_wgrad_desc d = conv(ABC_BF16, 16, 384, 384, 16, 1, 3);
        d.dtype_q = ABC_F32; d.q.scale = d.q.shift = d.q.slope = nullptr;
        show("one-channel stem 16 x 1 at 384 x 384", d);
    }
    {
        abc_wgrad_desc d = conv(ABC_BF16, 16, 96, 96, 360, 128, 1);
        d.dtype_p = ABC_F32; d.p.planar = 1; d.p.ctot = 360; d.p.ldx = 360;
        show("a head's 1x1, 360 channels", d);
    }
    return 0;
}
