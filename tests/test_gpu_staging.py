"""GPU tier of contract.PinnedStaging through its three users: two loads in a row without a host synchronisation in between
must leave the SECOND load on the device, and each run() must have read the load in front of it -- the pinned buffers are
reused, so a load that did not wait for the previous copy, or a copy that was not ordered in front of the launch, shows as
the other batch's records.  The smallest shapes at which that shows; results are read after one synchronize()."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import abcnet_amd  # noqa: E402,F401
from abcnet_amd.augment import ImageBuilder, param_row, test_ink_max as ink_max  # noqa: E402
from abcnet_amd.ops import GraphScore  # noqa: E402
from abcnet_amd.raster import TargetRasterizer, parse_record  # noqa: E402
from oracle import raster_oracle as ro  # noqa: E402

DEV = "cuda"
H = 8      # head-map cells: annotation coordinates 0 .. 31
# per image (atoms "El:x,y,charge[,hs];", bonds "order:x,y,dx,dy,stereo,direction;"); A and B differ in every image and in their counts
NOTES_A = [("C:4,4,0,1;N:20,12,1;O:28,28,-1,0;", "1:12,8,8,4,0,0;2:24,20,4,8,0,0;"),
           ("Cl:16,16,0;", "")]
NOTES_B = [("S:8,24,0;", "3:8,20,0,4,0,0;"),
           ("C:0,0,0,0;C:31,31,0;N:12,20,1,1;Br:24,4,0;", "1:6,6,6,6,0,0;1:20,12,8,-8,1,1;4:18,26,6,-6,0,0;1:28,16,-4,12,6,0;")]


def _maps(rz):
    return [t.cpu().numpy() for t in rz.targets]


def _check_raster(rz, maps, notes):
    recs = [parse_record(a, q, h=H) for a, q in notes]
    for b, (a, q) in enumerate(notes):
        want = ro.rasterize(a, q, h=H)
        for mi in range(8):
            assert maps[mi].dtype == want[mi].dtype and np.array_equal(maps[mi][b], want[mi]), (b, mi)
    assert rz.d_cnt.cpu().tolist() == [[len(r[0]) for r in recs], [len(r[1]) for r in recs]]
    for b, (a, q, r) in enumerate(recs):
        assert np.array_equal(rz.d_atoms[b, :len(a)].cpu().numpy(), a) and np.array_equal(rz.d_bonds[b, :len(q)].cpu().numpy(), q)
        assert np.array_equal(rz.d_rho[b, :len(q)].cpu().numpy(), r)


@pytest.mark.parametrize("sparse", [False, True])
def test_rasteriser_draws_the_load_in_front_of_each_run(sparse):
    rec_a, rec_b = ([parse_record(a, q, h=H) for a, q in notes] for notes in (NOTES_A, NOTES_B))
    assert rec_a[0][0].tolist() != rec_b[0][0].tolist() and [len(r[0]) for r in rec_a] != [len(r[0]) for r in rec_b]
    rz = TargetRasterizer(2, H, H, max_atoms=4, max_bonds=4, sparse=sparse)
    rz.load(rec_a)
    rz.run()
    first = [t.clone() for t in rz.targets]      # (a device copy in stream order: no host synchronisation)
    rz.load(rec_b)
    rz.run()
    torch.cuda.synchronize()
    _check_raster(rz, _maps(rz), NOTES_B)
    for b, (a, q) in enumerate(NOTES_A):         # the first run drew the first load, not the second
        want = ro.rasterize(a, q, h=H)
        assert all(np.array_equal(first[mi][b].cpu().numpy(), want[mi]) for mi in range(8)), b
    # two loads, one run: the second load waits for the first one's copies and replaces them
    rz.load(rec_a)
    rz.load(rec_b)
    rz.run()
    torch.cuda.synchronize()
    _check_raster(rz, _maps(rz), NOTES_B)


def test_rasteriser_refuses_a_record_over_capacity_before_it_touches_the_staging():
    rz = TargetRasterizer(2, H, H, max_atoms=4, max_bonds=4)
    rec_b = [parse_record(a, q, h=H) for a, q in NOTES_B]
    rz.load(rec_b)
    big = parse_record("C:0,0,0;C:4,4,0;C:8,8,0;C:12,12,0;C:16,16,0;", "", h=H)
    with pytest.raises(ValueError):
        rz.load([rec_b[1], big])
    assert rz.h_cnt.tolist() == [[len(r[0]) for r in rec_b], [len(r[1]) for r in rec_b]]      # (row 0 was valid, and was not staged)
    rz.run()
    torch.cuda.synchronize()
    _check_raster(rz, _maps(rz), NOTES_B)


def test_graph_score_holds_the_second_load():
    # two molecules of the assembler's layout (ends 1-based); what they score is test_gpu_graphscore.py's subject
    cnt = torch.tensor([[3, 2, 0, 0], [2, 1, 0, 0]], dtype=torch.int32, device=DEV)
    atoms = torch.tensor([[[1, 1, 1, 0, -1], [3, 1, 2, 0, -1], [3, 5, 3, 0, -1], [0, 0, 0, 0, 0]],
                          [[2, 2, 1, 0, -1], [6, 6, 1, 0, -1], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]], dtype=torch.int32, device=DEV)
    bonds = torch.tensor([[[1, 2, 1, 0], [2, 3, 2, 1], [0, 0, 0, 0], [0, 0, 0, 0]],
                          [[1, 2, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]], dtype=torch.int32, device=DEV)
    gs = GraphScore(cnt, atoms, bonds, max_atoms=4, max_bonds=4)
    assert not gs.loaded
    rec_a = [(np.array([[1, 1, 1, 0], [3, 1, 2, 0], [3, 5, 3, 0], [7, 7, 1, 1]], np.int32), np.array([[0, 1, 1], [1, 2, 2], [2, 3, 1]], np.int32)),
             (np.array([[5, 5, 6, 0]], np.int32), np.zeros((0, 3), np.int32))]
    rec_b = [(np.array([[2, 2, 1, 0], [6, 6, 1, 0]], np.int32), np.array([[0, 1, 1]], np.int32))]      # one record: row 1 becomes empty
    for loads in ((rec_a, "run", rec_b, "run"), (rec_a, rec_b, "run")):
        for item in loads:
            if item == "run":
                gs.run()
            else:
                gs.load(item)
        torch.cuda.synchronize()
        assert gs.loaded
        (h_atoms, h_bonds, _), (d_atoms, d_bonds, d_cnt) = gs.records.staging.host.values(), gs.records.staging.dev.values()
        assert d_cnt.cpu().tolist() == [[2, 0], [1, 0]]
        assert d_atoms[0, :2].cpu().tolist() == rec_b[0][0].tolist() and d_bonds[0, :1].cpu().tolist() == rec_b[0][1].tolist()
        assert torch.equal(d_atoms.cpu(), h_atoms) and torch.equal(d_bonds.cpu(), h_bonds)


def test_image_builder_holds_the_second_load():
    S = 8
    rng = np.random.RandomState(5)
    img_a = [rng.randint(0, 256, (S, S)).astype(np.uint8) for _ in range(2)]
    img_b = [(255 - a) for a in img_a]
    ib = ImageBuilder(2, S, "test")
    want_par = np.stack([param_row((S, S), None, S)] * 2)
    for loads in ((img_a, "run", img_b, "run"), (img_a, img_b, "run")):
        for item in loads:
            if item == "run":
                ib.run()
            else:
                ib.load(item)
        torch.cuda.synchronize()
        assert np.array_equal(ib.d_par.cpu().numpy(), want_par) and np.array_equal(ib.h_par.numpy(), want_par)
        assert np.array_equal(ib.d_src[:, :S, :S].cpu().numpy(), np.stack(img_b))
        # utils_for_test.py:22-24: ink where the byte is at most the threshold
        assert np.array_equal(ib.out[:, 0].cpu().numpy(), (np.stack(img_b) <= ink_max()).astype(np.float32))
