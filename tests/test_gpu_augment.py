"""The device input-image builder (csrc/augment.hip through abcnet_amd.augment) against the reference's goldens (noise off), the
numpy oracle with the hash mirror (noise on), the noise statistics, guard bands, and whole Trainer / InferenceRunner steps fed by it."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abcnet_amd  # noqa: E402,F401
from abcnet_amd import _lib as L  # noqa: E402
from abcnet_amd.augment import AugmentDraw, ImageBuilder, SampleBuilder, draw_augment, noise_threshold  # noqa: E402
import augment_oracle as ao  # noqa: E402

DEV = "cuda"


def _bits(a, S=512):
    return np.unpackbits(a)[:S * S].reshape(S, S).astype(bool)


def _quiet(rows, cols, ddx, ddy, key=0):
    return AugmentDraw(rows, cols, ddx, ddy, 1, 1, 0.0, 0.0, key)


def test_amount0_matches_train_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "augment_512.npz"))
    cases = [ci for ci in range(int(g["n"])) if float(g["c%d_amount" % ci]) == 0]
    srcs = [g["c%d_src" % ci] for ci in cases]
    draws = [_quiet(*(int(v) for v in g["c%d_geom" % ci])) for ci in cases]
    ib = ImageBuilder(len(cases), 512, "train", max_src=(512, 512))
    ib.load(srcs, draws)
    out = ib.run().cpu().numpy()
    for k, ci in enumerate(cases):
        np.testing.assert_array_equal(out[k, 0], _bits(g["c%d_out" % ci]).astype(np.float32), err_msg=str(g["c%d_tag" % ci]))


def test_test_mode_matches_test_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "augment_test_512.npz"))
    n = int(g["n"])
    ib = ImageBuilder(n, 512, "test")
    ib.load([g["c%d_src" % ci] for ci in range(n)])
    out = ib.run().cpu().numpy()
    for ci in range(n):
        np.testing.assert_array_equal(out[ci, 0], _bits(g["c%d_out" % ci]).astype(np.float32))


@pytest.mark.parametrize("S", [384, 512])
def test_amount0_matches_oracle_on_other_sizes(S):
    """S = 384 and non-square sources (a padded 300 x 450, resizes up and down on either axis, a row that lands at ddy odd)"""
    shapes_geoms = [((300, 450), (300, 450, (S - 300) // 2, (S - 450) // 2)), ((S, S), (int(0.83 * S), S, 0, 0)),
                    ((S, S), (S, int(0.91 * S), 0, 5)), ((201, 333), (S - 3, S - 7, 1, 3)), ((S - 1, S - 9), (S - 1, S - 9, 1, 9))]
    shapes_geoms = [(sh, gm) for sh, gm in shapes_geoms if gm[0] + gm[2] <= S and gm[1] + gm[3] <= S]
    srcs = [ao.fixture_render(70 + i, *sh) for i, (sh, _) in enumerate(shapes_geoms)]
    draws = [_quiet(*gm) for _, gm in shapes_geoms]
    ib = ImageBuilder(len(srcs), S, "train", max_src=(512, 512))
    ib.load(srcs, draws)
    out = ib.run().cpu().numpy()
    for k, (src, dr) in enumerate(zip(srcs, draws)):
        want = ao.ink_train(src, S, dr.rows, dr.cols, dr.ddx, dr.ddy).astype(np.float32)
        np.testing.assert_array_equal(out[k, 0], want, err_msg="case %d %s" % (k, dr))


def test_resizes_round_every_multiply_and_add():
    """sources whose resize lands within an ulp of the threshold: a uniform 153 resized to 512 x 450 or 450 x 512 interpolates to
    152.99998 (ink) when every product and sum is rounded on its own and to 153.0 (no ink) when a multiply-add is fused -- a whole
    column / row of difference (tests/test_augment_host.py shows both verdicts); plus a 152 / 153 / 154 mix resized both ways"""
    S = 512
    rs = np.random.RandomState(11)
    mix = rs.choice(np.array([152, 153, 154], np.uint8), size=(512, 512))
    cases = [(np.full((512, 512), 153, np.uint8), (512, 450, 0, 31)), (np.full((512, 512), 153, np.uint8), (450, 512, 31, 0)),
             (mix, (512, 450, 0, 31)), (mix, (450, 512, 31, 0)), (mix, (479, 433, 16, 39))]
    ib = ImageBuilder(len(cases), S, "train", max_src=(512, 512))
    ib.load([c[0] for c in cases], [_quiet(*c[1]) for c in cases])
    out = ib.run().cpu().numpy()
    for k, (src, gm) in enumerate(cases):
        want = ao.ink_train(src, S, *gm).astype(np.float32)
        np.testing.assert_array_equal(out[k, 0], want, err_msg="case %d %s" % (k, gm))
    assert out[0, 0].sum() == 512 and out[1, 0].sum() == 512


def test_run_replays_from_a_captured_graph():
    """ImageBuilder.run() captured once; later loads replay it with the new images and parameters"""
    S, B = 256, 4
    ib = ImageBuilder(B, S, "train", amount=0.2, max_src=(S, S))
    rs = np.random.RandomState(5)

    def batch(seed):
        srcs = [ao.fixture_render(seed + b, S - 8 * b, S - 16 * b) for b in range(B)]
        draws = [draw_augment(rs, 0.2, s.shape, S)[0] for s in srcs]
        draws[0] = draws[0]._replace(rows=201, ddx=27)
        return srcs, draws
    srcs, draws = batch(700)
    ib.load(srcs, draws)
    ib.run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ib.run()
    for seed in (710, 720):
        srcs, draws = batch(seed)
        ib.load(srcs, draws)
        ib.out.fill_(-1.0)
        g.replay()
        out = ib.out.cpu().numpy()
        for b in range(B):
            np.testing.assert_array_equal(out[b, 0], ao.build_train(srcs[b], S, draws[b]), err_msg="seed %d image %d" % (seed, b))


@pytest.mark.parametrize("B", [16, 5])
def test_noise_matches_hash_oracle(B):
    S = 512
    rs = np.random.RandomState(100 + B)
    shapes = [[(512, 512), (400, 460), (300, 450), (512, 500)][b % 4] for b in range(B)]
    srcs = [ao.fixture_render(200 + b, *sh) for b, sh in enumerate(shapes)]
    ib = ImageBuilder(B, S, "train", amount=0.2, max_src=(512, 512))
    draws = [dr for dr, _ in (draw_augment(rs, 0.2, sh, S) for sh in shapes)]
    if not any(dr.rows != sh[0] or dr.cols != sh[1] for dr, sh in zip(draws, shapes)):
        draws[0] = draws[0]._replace(rows=451, ddx=30)            # at least one resize in the batch
    ib.load(srcs, draws)
    out = ib.run().cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(out[b, 0], ao.build_train(srcs[b], S, draws[b]), err_msg="image %d %s" % (b, draws[b]))


def _run_one(ib, src, dr):
    ib.load([src] * ib.B, [dr] * ib.B)
    return ib.run()[0, 0].cpu().numpy().astype(bool)


def _lag1(f):
    x = f.astype(np.float64) - f.mean()
    den = (x * x).sum()
    return (x[:, 1:] * x[:, :-1]).sum() / den, (x[1:, :] * x[:-1, :]).sum() / den


def test_noise_statistics():
    S = 512
    n = S * S
    ib = ImageBuilder(1, S, "train")
    white = np.full((S, S), 255, np.uint8)
    black = np.zeros((S, S), np.uint8)
    for i, (salt, pepper) in enumerate([(0.002, 0.05), (0.0007, 0.19), (0.001, 0.5)]):
        key = 0x9E3779B97F4A7C15 * (i + 1) & ((1 << 64) - 1)
        s_field = _run_one(ib, white, AugmentDraw(S, S, 0, 0, 1, 1, salt, 0.0, key))            # salt only
        p_field = ~_run_one(ib, black, AugmentDraw(S, S, 0, 0, 1, 1, 0.0, pepper, key))         # pepper only
        for f, r in ((s_field, salt), (p_field, pepper)):
            sigma = np.sqrt(n * r * (1 - r))
            assert abs(f.sum() - n * r) < 6 * sigma, (f.sum(), n * r)
            ah, av = _lag1(f)
            assert abs(ah) < 6 / np.sqrt(n) and abs(av) < 6 / np.sqrt(n), (ah, av)
        # same key: same output; another key: about 2 r (1 - r) n pixels change
        again = ~_run_one(ib, black, AugmentDraw(S, S, 0, 0, 1, 1, 0.0, pepper, key))
        np.testing.assert_array_equal(again, p_field)
        other = ~_run_one(ib, black, AugmentDraw(S, S, 0, 0, 1, 1, 0.0, pepper, key ^ (1 << 40)))
        q = 2 * pepper * (1 - pepper)
        assert abs((other != p_field).sum() - n * q) < 6 * np.sqrt(n * q * (1 - q))


def test_guard_bands_and_source_padding():
    """out lives between sentinel bands; the staging bytes beyond each source's width (inside the pitch) and below its height are set
    to black: neither band changes and the output still equals the oracle, so the kernel reads only the source's own bytes"""
    S, B, pad = 384, 3, 4096
    big = torch.full((2 * pad + B * S * S,), 7.25, dtype=torch.float32, device=DEV)
    out = big[pad:pad + B * S * S].view(B, 1, S, S)
    ib = ImageBuilder(B, S, "train", out=out, max_src=(400, 470))
    shapes = [(300, 450), (384, 370), (257, 301)]
    geoms = [(300, 330, 40, 27), (384, 370, 0, 7), (383, 384, 0, 0)]
    srcs = [ao.fixture_render(400 + b, *sh) for b, sh in enumerate(shapes)]
    draws = [AugmentDraw(*gm, 1, 1, 0.001, 0.05, 1234567 + b) for b, gm in enumerate(geoms)]
    ib.load(srcs, draws)
    for b, (h, w) in enumerate(shapes):
        ib.d_src[b, :, w:] = 0
        ib.d_src[b, h:, :] = 0
    src_before = ib.d_src.clone()
    ib.run()
    torch.cuda.synchronize()
    assert bool((big[:pad] == 7.25).all()) and bool((big[pad + B * S * S:] == 7.25).all())
    assert torch.equal(ib.d_src, src_before)
    got = out.cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(got[b, 0], ao.build_train(srcs[b], S, draws[b]))


def test_refusals():
    with pytest.raises(L.AbcNetHipError):
        ImageBuilder(2, 64, "train", out=torch.zeros((2, 3, 64, 64), device=DEV))       # a 3-channel model's input
    with pytest.raises(L.AbcNetHipError):
        ImageBuilder(2, 64, "train", out=torch.zeros((2, 1, 64, 64), device=DEV, dtype=torch.float16))
    ib = ImageBuilder(1, 64, "train")
    with pytest.raises(ValueError):
        ib.load([np.zeros((64, 64), np.uint8)], [_quiet(65, 64, 0, 0)])
    with pytest.raises(ValueError):
        ib.load([np.zeros((80, 64), np.uint8)], [_quiet(64, 64, 0, 0)])
    with pytest.raises(L.AbcNetHipError):
        ib.run()                                          # nothing loaded: the staged parameters are refused
    it = ImageBuilder(1, 64, "test")
    with pytest.raises(ValueError):
        it.load([np.zeros((32, 64), np.uint8)])


HEADS = [1, 14, 3, 2, 1, 360, 60, 60]


def test_trainer_fed_by_sample_builder_is_bit_identical():
    from abcnet_amd.raster import TargetRasterizer, parse_record
    from abcnet_amd.synthetic import random_annotations
    from abcnet_amd.train import Trainer
    from abcnet_amd.unet import UNet
    B, S = 16, 384
    trs = []
    for _ in range(2):
        torch.manual_seed(0)
        m = UNet(1, HEADS, dtype="bf16").to(DEV)
        trs.append(Trainer(m, B, S, S, use_graph=False))
    ta, tb = trs
    sb = SampleBuilder(ta, amount=0.1, max_src=(S, S), sparse=True, max_atoms=64, max_bonds=64)
    rz = TargetRasterizer(B, S // 4, max_atoms=64, max_bonds=64, targets=tb.targets, sparse=True)
    tb.use_sparse_targets(rz)
    for step in range(3):
        srcs = [ao.fixture_render(1000 + 16 * step + b, S - 16 * (b % 3), S - 8 * (b % 5)) for b in range(B)]
        ann = [random_annotations(20, 22, 500 + 16 * step + b, size=300) for b in range(B)]
        rs_a, rs_b = np.random.RandomState(step), np.random.RandomState(step)
        draws = sb.load(srcs, [a for a, _ in ann], [q for _, q in ann], rs_a)
        imgs, recs = [], []
        for b in range(B):
            dr, offs = draw_augment(rs_b, 0.1, srcs[b].shape, S)
            assert dr == draws[b]
            imgs.append(ao.build_train(srcs[b], S, dr))
            recs.append(parse_record(ann[b][0], ann[b][1], *offs, h=S // 4))
        sb.run()
        ta.step()
        tb.load_batch(torch.from_numpy(np.stack(imgs)[:, None]).to(DEV))
        rz.load(recs)
        rz.run()
        tb.step()
        torch.cuda.synchronize()
        assert torch.equal(ta.input_images, tb.input_images), step
        assert ta.loss_value() == tb.loss_value(), step
        assert torch.equal(ta.model._flat_grad, tb.model._flat_grad), step


def test_inference_fed_by_test_mode_builder_is_bit_identical():
    from abcnet_amd.infer import InferenceRunner
    from abcnet_amd.unet import UNet
    from oracle import unet_oracle as uo
    B, S = 2, 256
    m = UNet(1, HEADS, dtype="bf16")
    m.load_state_dict(uo.filled_state("unet", 1, HEADS, seed=0))
    m = m.to(DEV)
    ir = InferenceRunner(m, B, S, S, use_graph=False)
    ib = ImageBuilder(B, S, "test", out=ir.input_images)
    srcs = [ao.fixture_render(600 + b, S, S) for b in range(B)]
    ib.load(srcs)
    ib.run()
    ir.step()
    got = [t.clone() for t in (ir.atom_mask, ir.bond_mask, ir.rho_abs, ir.omega_mask)]
    ir.load_batch(torch.from_numpy(np.stack([ao.build_test(s) for s in srcs])[:, None]).to(DEV))
    ir.step()
    torch.cuda.synchronize()
    for a, b in zip(got, (ir.atom_mask, ir.bond_mask, ir.rho_abs, ir.omega_mask)):
        assert torch.equal(a, b)
