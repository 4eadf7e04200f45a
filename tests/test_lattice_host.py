"""CPU tier of the exact-sum tests: the lattice helper catches what the relative-to-max bar lets through, and the case tables of
tests/test_gpu_exact.py (kept in tests/lattice.py) reach every weight-gradient family, tile, patch height, loader and K-step form and
every convolution kernel -- settled here through the host-side routing queries, before any kernel runs."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import abcnet_amd  # noqa: F401
from abcnet_amd import _lib as L
from abcnet_amd.engine import taps_square

import hiputil as U
import lattice as T


def _case(table, id):
    return next(c for c in table if c["id"] == id)


def test_lattice_draws_are_exact_in_bf16_through_every_transform():
    g = T.gen(1)
    x, y = T.draw_data(g, (2, 64, 9, 11)), T.draw_data(g, (2, 64, 9, 11))
    T.assert_bf16_exact(x)
    for _ in range(8):
        T.assert_bf16_exact(T.act(x, *T.draw_coef(g, 64)), "act")
        T.assert_bf16_exact(T.dual(x, y, *T.draw_dual(g, 64)), "dual")
    xc = T.draw_data(g, (2, 64, 9, 11), coarse=True)
    T.assert_bf16_exact(T.act(xc, *T.draw_coef(g, 64, coarse=True)), "coarse act")
    T.assert_bf16_exact(T.draw_weight(g, (8, 8, 3, 3)))
    with pytest.raises(AssertionError):
        T.assert_bf16_exact(torch.tensor([1.0 + 2.0 ** -8]))
    with pytest.raises(AssertionError):
        T.assert_bf16_exact(torch.tensor([2.0 ** -9]))         # exact in bf16, but off the 1 / 256 lattice
    with pytest.raises(AssertionError):
        T.assert_budget(torch.tensor([2.0 ** 15]))             # 2^23 units: half the range


def test_reference_weight_gradient_is_torchs_and_f32_is_exact_under_the_budget():
    """wgrad_ref (the header's formula, one einsum per tap) against autograd of conv2d in f64, and torch's f32 weight gradient
    bit-equal to both: under the asserted budget f32 sums are exact in any order"""
    c = _case(T.WG_CASES, "pm1-prefetch")
    o = T.wg_data(c)
    assert o["budget"] < 0.5
    w = torch.zeros((c["Ca"], c["Cb"], 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv2d(o["Q"].double(), w, None, padding=1).backward(o["P"].double())
    assert torch.equal(o["ref"].view(c["Ca"], c["Cb"], 3, 3), w.grad)
    w32 = torch.zeros((c["Ca"], c["Cb"], 3, 3), requires_grad=True)
    F.conv2d(o["Q"], w32, None, padding=1).backward(o["P"])
    assert torch.equal(w32.grad.double(), w.grad)
    assert torch.equal(T.wgrad_ref(o["P"], o["Q"], taps_square(3), 1, torch.float32).double(), o["ref"])
    # stride 2 (ConvTranspose): against autograd of conv_transpose2d + the crop of the first row and column
    c = _case(T.WG_CASES, "2x1-convT-12")
    o = T.wg_data(c)
    wt = torch.zeros((c["Ca"], c["Cb"], 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv_transpose2d(o["P"].double(), wt, None, stride=2)[:, :, 1:, 1:].backward(o["Q"].double())
    assert torch.equal(o["ref"].view(c["Ca"], c["Cb"], 3, 3), wt.grad)


def test_a_lost_pixel_column_passes_the_old_bar_and_fails_the_exact_one():
    """a 2 x 24 x 40 weight gradient with the last pixel column missing from one tap: every element of that tap loses 1 / 40 of
    its terms.  With operands of one sign (k / 4 in [1, 2] here) that is 2.5 % of every element:
    relerr() < 3e-2 -- the bar of tests/test_gpu_kernels.py -- passes it; equality does not, and says where.  (On the zero-mean
    lattice of the GPU cases the same mutant is 12 % of the maximum at this size and shrinks with the map: also recorded here.)"""
    g = T.gen(7)
    P, Q = 1.5 + T.draw(g, (2, 32, 24, 40), 4, 2), 1.5 + T.draw(g, (2, 32, 24, 40), 4, 2)        # k / 4 in [1, 2]
    T.assert_bf16_exact(P)
    taps = taps_square(3)
    T.assert_budget(T.wgrad_ref(P, Q, taps), "self-check")
    ref = T.wgrad_ref(P, Q, taps)
    want = T.expect(ref, T.F32)
    T.assert_wgrad_equal(want.clone(), want)
    tap = 4                                                    # the centre tap: P's last column meets Q's last column
    lost = torch.einsum("nah,nbh->ab", P[:, :, :, -1].double(), Q[:, :, :, -1].double())
    mutant = ref.clone()
    mutant[:, :, tap] -= lost
    assert 2e-2 < U.relerr(mutant, ref) < 3e-2, "the old bar was expected to let this through"
    with pytest.raises(AssertionError) as e:
        T.assert_wgrad_equal(mutant.float(), want, "lost column")
    by_tap = [0] * 9
    by_tap[tap] = 32 * 32
    assert "1024 of 9216" in str(e.value) and "by tap: %s" % by_tap in str(e.value)
    c = _case(T.WG_CASES, "pm1-prefetch")
    assert (c["B"], c["H"], c["W"]) == (2, 24, 40)
    o = T.wg_data(c)
    zm = o["ref"].clone()
    zm[:, :, tap] -= torch.einsum("nah,nbh->ab", o["P"][:, :, :, -1].double(), o["Q"][:, :, :, -1].double())
    assert 3e-2 < U.relerr(zm, o["ref"]) < 0.2
    # an unwritten slab element: stale data in training, zero in a test that clears the slabs -- NaN here
    stale = want.clone()
    stale[5, 7, 2] = float("nan")
    with pytest.raises(AssertionError, match=r"1 of 9216 .*\(1 not finite\)"):
        T.assert_wgrad_equal(stale, want)


def test_a_lost_border_term_passes_the_old_bar_and_fails_the_exact_one():
    """a 32 -> 16 3 x 3 convolution (K = 288) that drops one (tap, channel) term in the last image column: with operands of one sign
    1 / 288 of those outputs.  The GPU case of the same layer (zero-mean lattice) is recorded next to it: 3.7 % of the maximum there,
    and 1 / 4 of that at K = 1152 or on a map whose outputs are four times larger"""
    g = T.gen(8)
    B, Cin, Cout, H, W = 2, 32, 16, 20, 40
    x, w = 1.5 + T.draw(g, (B, Cin, H, W), 4, 2), 0.75 + T.draw(g, (Cout, Cin, 3, 3), 8, 2)
    T.assert_bf16_exact(x)
    T.assert_bf16_exact(w)
    T.assert_budget(F.conv2d(x.double(), w.double(), None, padding=1), "self-check")
    ref = F.conv2d(x.double(), w.double(), None, padding=1)
    mutant = ref.clone()
    # tap (0, -1) of channel 0 at the outputs of column W - 1 reads column W - 2
    mutant[:, :, :, -1] -= w[:, 0, 1, 0].double().view(1, -1, 1) * x[:, 0, :, -2].double().unsqueeze(1)
    for dt in (T.F32, T.BF16):
        want, got = T.expect(ref, dt), T.expect(mutant, dt)
        T.assert_conv_equal(want.clone(), want)
        assert U.relerr(got, ref) < U.tol(dt, 3e-2, 3e-2), "the old bar was expected to let this through"
        with pytest.raises(AssertionError) as e:
            T.assert_conv_equal(got, want, "lost border term")
        msg = str(e.value)
        n = int((got != want).sum())
        assert (n == B * Cout * H if dt == T.F32 else n > 100) and "%d on the image border" % n in msg
        assert "by column %% 16: %s" % ([0] * 7 + [n] + [0] * 8) in msg      # column 39 = 2 * 16 + 7
    c = _case(T.CONV_CASES, "narrow-32to16")
    o = T.conv_data(c)
    zm = o["ref"].clone()
    zm[:, :, :, -1] -= o["w"][:, 0, 1, 0].double().view(1, -1, 1) * o["xin"][:, 0, :, -2].double().unsqueeze(1)
    assert 1e-2 < U.relerr(zm, o["ref"]) < 5e-2


def test_expect_rounds_to_nearest_even():
    r = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -16], dtype=torch.float64)
    assert T.expect(r, T.BF16).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]
    assert torch.equal(T.expect(r, T.F32).double(), r)


def test_case_ids_are_unique():
    for table in (T.WG_CASES, T.CONV_CASES):
        ids = [c["id"] for c in table]
        assert len(set(ids)) == len(ids)


def test_every_case_is_inside_its_budget_and_exact_in_bf16():
    """wg_data / conv_data assert both; here so that a wrong case is found before any GPU visit"""
    worst = max(T.wg_data(c)["budget"] for c in T.WG_CASES)
    worst_c = max(max(o["budget"], o.get("stats_budget", 0.0)) for o in map(T.conv_data, T.CONV_CASES))
    assert 0.0 < worst < 0.5 and 0.0 < worst_c < 0.5
    assert sum(T.wg_data(c)["budget"] > 0.1 for c in T.WG_CASES) >= 8         # (not vacuous: many cases use a good part of the range)


def test_case_tables_reach_every_route():
    """every case's descriptor through abc_wgrad_route_info / abc_conv_variant: each is served as its table row says, and together
    the rows reach every family, tile, patch height, loader, K-step form and segment-table state that the kernels have"""
    lib = L.load()
    routes, fuses = [], set()
    for c in T.WG_CASES:
        for ns in c["nsplit"]:
            d = T.wg_desc(c, ns)
            r = T.wg_route(lib, d)
            assert r == c["route"], (c["id"], r)
            at, bt = L.i32(), L.i32()
            L.check(lib.abc_wgrad_tile(C.byref(d), C.byref(at), C.byref(bt)), "tile")
            assert (at.value, bt.value) == r[1:3], c["id"]
            if c["dual"]:
                assert lib.abc_wgrad_fuses_apply(C.byref(d)) == 1, c["id"]
                fuses.add((r[0], r[4], r[6]))
        routes.append((c, r))
    fam = {r[0] for _, r in routes}
    assert fam == {T.HEAD, T.C1, T.NARROW16, T.N32R2, T.GENERAL}
    gen = [(c, r) for c, r in routes if r[0] == T.GENERAL]
    stride = lambda c: 2 if c["kind"] == "convT" else 1
    assert {(r[1], r[2], stride(c)) for c, r in gen} == {(4, 2, 1), (2, 2, 1), (1, 4, 1), (2, 1, 2), (1, 1, 1), (1, 1, 2)}
    assert {r[3] for _, r in gen} == {1, 2, 4}                 # pm
    assert {r[4] for _, r in gen} == {0, 1}                    # ts
    assert {r[5] for _, r in gen} == {0, 1}                    # fast
    assert {r[6] for _, r in gen} == {0, 1}                    # k3
    assert {(r[1], r[2], r[7]) for _, r in gen if r[1] * r[2] >= 4 and r[1] > 1} == {(2, 2, 0), (2, 2, 1), (4, 2, 0), (4, 2, 1)}
    # the BatchNorm-backward correction on load: the general kernel's static 3x3 step and its tap-split form, and the three others
    assert fuses >= {(T.GENERAL, 0, 1), (T.GENERAL, 1, 0), (T.NARROW16, 0, 0), (T.N32R2, 0, 0), (T.C1, 0, 0)}
    assert any(c["dual"] and r[7] for c, r in gen) and any(c["dual"] and r[3] == 4 for c, r in gen)
    # both compute modes, operand slices, every split count at least once next to the patch count
    assert {c["dt"] for c, _ in routes} == {T.F32, T.BF16}
    # convolutions
    seen = set()
    for c in T.CONV_CASES:
        for i, dt in enumerate((T.F32, T.BF16)):
            if c["variant"][i] is None:
                continue
            d = T.conv_desc_host(c, dt)
            v, lay = lib.abc_conv_variant(C.byref(d)), lib.abc_conv_weight_layout(C.byref(d))
            assert (v, lay) == (c["variant"][i], c["layout"][i]), (c["id"], dt, v, lay)
            info = (C.c_int32 * 7)(*([-7] * 7))
            assert lib.abc_conv_route_info(C.byref(d), info) == 0, (c["id"], dt)
            assert tuple(info[:2]) == (c["variant"][i], c["layout"][i]), (c["id"], dt, tuple(info))
            seen.add((v, lay))
    assert seen == {(0, 0), (1, 0), (1, 1), (2, 0), (5, 0)}
    for a in T.CONVT_FUSED_CASES:
        assert lib.abc_convt_fused_ok(C.byref(T.convt_desc_host(*a))) == 1, a


def test_route_info_agrees_with_the_other_queries_on_the_recorded_plans(golden_dir):
    """abc_wgrad_route_info over every descriptor of tests/golden/wgrad_routes.json: its tile is abc_wgrad_tile's, its family follows
    from the tile code, and the fields of the general kernel are zero for the other families"""
    import json
    import os
    with open(os.path.join(golden_dir, "wgrad_routes.json")) as f:
        tab = json.load(f)
    cols, lib = tab["columns"], L.load()
    nf = cols.index("taps")
    fam_of = {(0, 0): T.HEAD, (0, 1): T.C1, (0, 2): T.NARROW16, (0, 3): T.N32R2}
    for row in tab["rows"]:
        d = L.WgradDesc()
        fields = [(d, n, x) for n, x in zip(cols[2:nf], row[2:])]
        fields += [(getattr(d, o), n, x) for o, i in zip("pq", row) for n, x in zip(tab["operand"], tab[o][i])]
        for o, n, x in fields:
            if dict(o._fields_)[n] is C.c_void_p:
                x = T.DUMMY if x else None
            setattr(o, n, x)
        for i, (dy, dx) in enumerate(zip(*tab["taps"][row[nf]])):
            d.tap_dy[i], d.tap_dx[i] = dy, dx
        at, bt = row[cols.index("at")], row[cols.index("bt")]
        info = (C.c_int32 * 8)(*([-7] * 8))
        rc = lib.abc_wgrad_route_info(C.byref(d), info)
        assert rc == row[cols.index("tile_rc")]
        if rc:
            continue
        r = tuple(info)
        assert r[1:3] == (at, bt) and r[0] == fam_of.get((at, bt), T.GENERAL)
        if r[0] != T.GENERAL:
            assert r[3:] == (0, 0, 0, 0, 0)
        else:
            assert r[3] in (1, 2, 4) and all(v in (0, 1) for v in r[4:])
