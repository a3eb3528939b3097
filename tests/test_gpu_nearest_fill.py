"""ops.nearest_fill on the GPU (run with -m gpu): exact equality with the brute-force numpy oracle (nearest_fill_np.py), words
compared as int32, on the smallest shapes at which the kernel can go wrong -- word boundaries inside a row, a partly filled
last word, a single row, every tie of the distance, the early-exit boundary, the full-height walk, frames without a seed -- and
propagate_maps(fill="nearest") end to end on a painted scene, without a model."""
import numpy as np
import pytest
import torch

import nearest_fill_np as NF
from c2m_amd import evaluate, interactive as I, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1, 1), (1, 70), (5, 64), (7, 65), (9, 130), (33, 300)]
RING = [(0, 5), (-3, 4), (3, -4), (4, 3), (-5, 0)]                     # all at distance 5
TIES = [[(0, 5), (0, -5)], [(5, 0), (-5, 0)],
        RING, RING[:2], [RING[0], RING[2], RING[3]], RING[2:4], [RING[0], RING[1], RING[3]], [RING[1], RING[4]], RING[1:4],
        [RING[0], RING[3], RING[4]],
        [(0, 5), (4, 3)],                                              # the same row wins over a row below
        [(0, 5), (-5, 0)]]                                             # straight above at dy = 5: the early-exit boundary
NAN_WORD = 0xFFC12345 - 2 ** 32                                        # a negative quiet NaN with a payload, as an int32 word


def words(rng, *shape):
    """Random 32-bit patterns: NaN payloads, infinities, denormals, negative ids."""
    return rng.integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)


def fill(hole, seed, pf=None, pi=None):
    """hole, seed [B,T,H,W] numpy; pf / pi int32 words [B,C,T,H,W] or None -> (filled pf words, filled pi, unfilled) from the GPU."""
    d = lambda a, dt: None if a is None else torch.from_numpy(np.array(a)).view(dt).to(DEV)
    tf, ti = d(pf, torch.float32), d(pi, torch.int32)
    unfilled = ops.nearest_fill(d(hole, torch.uint8), d(seed, torch.uint8), tf, ti)
    torch.cuda.synchronize()
    back = lambda t: None if t is None else t.cpu().view(torch.int32).numpy()
    return back(tf), back(ti), unfilled.cpu().numpy()


def check(hole, seed, pf, pi):
    """The GPU's result equals the oracle's, word for word; returns it."""
    got_f, got_i, unfilled = fill(hole, seed, pf, pi)
    (want_f, want_i), want_unfilled = NF.nearest_fill(hole, seed, [pf, pi])
    for got, want in ((got_f, want_f), (got_i, want_i)):
        assert (got is None) == (want is None)
        if got is not None:
            assert got.dtype == np.int32 and np.array_equal(got, want)
    assert unfilled.dtype == np.int32 and np.array_equal(unfilled, want_unfilled)
    return got_f, got_i, unfilled


def random_masks(rng, shape, p_hole, p_seed):
    hole = (rng.random(shape) < p_hole).astype(np.uint8)
    seed = ((rng.random(shape) < p_seed) & (hole == 0)).astype(np.uint8)
    return hole, seed


def index_plane(B, T, H, W):
    """int32 [B,1,T,H,W]: every pixel holds y * W + x, so a filled pixel names its source."""
    return np.broadcast_to(np.arange(H * W, dtype=np.int32).reshape(H, W), (B, 1, T, H, W)).copy()


# ------------------------------------------------------------------------------------------------ sizes and word boundaries
@pytest.mark.parametrize("size", SIZES)
def test_random_masks_at_the_edge_sizes(size):
    H, W = size
    rng = np.random.default_rng(H * 1000 + W)
    B, T = 2, 4
    hole, seed = random_masks(rng, (B, T, H, W), 0.4, 0.08)
    hole[0, 0], seed[0, 0] = 1, 0
    seed[0, 0, H - 1, W - 1], hole[0, 0, H - 1, W - 1] = 1, 0         # the last bit of a (partly filled) last word is the only seed
    hole[0, 1], seed[0, 1] = 1, 0
    seed[0, 1, 0, 0], hole[0, 1, 0, 0] = 1, 0
    hole[1, 0], seed[1, 0] = 1, 0                                      # nothing but holes
    hole[1, 1], seed[1, 1] = 0, 1                                      # nothing but seeds
    _, got_i, unfilled = check(hole, seed, words(rng, B, 3, T, H, W), index_plane(B, T, H, W))
    assert unfilled[1, 0] == H * W and unfilled[0, 0] == 0
    if H * W > 1:
        assert (got_i[0, 0, 0] == H * W - 1).all() and (got_i[0, 0, 1] == 0).all()


def test_padding_bits_are_never_seeds():
    """W = 70: the last word of a row holds 6 pixels.  Seeds only in column 0, holes at the right end: a padding bit read as a
    seed would be nearer than any true one."""
    H, W = 3, 70
    hole, seed = np.zeros((1, 1, H, W), np.uint8), np.zeros((1, 1, H, W), np.uint8)
    hole[..., 60:], seed[..., 0] = 1, 1
    _, got_i, _ = check(hole, seed, None, index_plane(1, 1, H, W))
    assert (got_i[0, 0, 0, :, 60:] == np.arange(H)[:, None] * W).all()


# ------------------------------------------------------------------------------------------------ ties
def test_ties_go_to_the_smaller_row_then_the_smaller_column():
    """One hole at (8, 62) of a 17 x 80 frame, so the candidates left and right of it lie in different words; one frame per
    case.  The id plane names the source: it must be the minimum of (d^2, y', x') whatever order the kernel visits rows in."""
    H, W, cy, cx = 17, 80, 8, 62
    masks = [NF.paint(H, W, cy, cx, seeds) for seeds in TIES]
    hole, seed = (np.stack([m[k] for m in masks])[None] for k in (0, 1))
    rng = np.random.default_rng(5)
    _, got_i, unfilled = check(hole, seed, words(rng, 1, 2, len(TIES), H, W), index_plane(1, len(TIES), H, W))
    assert not unfilled.any()
    for t, seeds in enumerate(TIES):
        dy, dx = min(seeds, key=lambda s: (s[0] ** 2 + s[1] ** 2, s[0], s[1]))
        assert got_i[0, 0, t, cy, cx] == (cy + dy) * W + cx + dx, seeds


def test_one_seed_in_a_far_corner():
    """Every other pixel is a hole: the full-height walk with the largest d^2, from each corner."""
    H, W = 33, 300
    hole, seed = np.ones((1, 4, H, W), np.uint8), np.zeros((1, 4, H, W), np.uint8)
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    for t, (y, x) in enumerate(corners):
        hole[0, t, y, x], seed[0, t, y, x] = 0, 1
    rng = np.random.default_rng(6)
    _, got_i, _ = check(hole, seed, words(rng, 1, 1, 4, H, W), index_plane(1, 4, H, W))
    for t, (y, x) in enumerate(corners):
        assert (got_i[0, 0, t] == y * W + x).all()


# ------------------------------------------------------------------------------------------------ what is left alone
def test_a_frame_without_a_seed_is_left_as_it_is():
    H, W = 9, 130
    rng = np.random.default_rng(7)
    hole, seed = random_masks(rng, (2, 3, H, W), 0.3, 0.05)
    seed[1, 1] = 0
    seed[0, 2] = hole[0, 2]                                            # set in both everywhere it is set at all: no seed either
    pf, pi = words(rng, 2, 4, 3, H, W), words(rng, 2, 1, 3, H, W)
    got_f, got_i, unfilled = check(hole, seed, pf, pi)
    for b, t in ((1, 1), (0, 2)):
        assert np.array_equal(got_f[b, :, t], pf[b, :, t]) and np.array_equal(got_i[b, :, t], pi[b, :, t])
        assert unfilled[b, t] == hole[b, t].sum() > 0
    assert unfilled.sum() == hole[1, 1].sum() + hole[0, 2].sum()       # zero for the other frames of the call


def test_pixels_that_are_neither_are_not_sources_and_not_written():
    H, W = 7, 65
    hole, seed = np.zeros((1, 1, H, W), np.uint8), np.zeros((1, 1, H, W), np.uint8)
    hole[0, 0, 3, 30:34] = 1                                           # surrounded by pixels that are neither
    seed[0, 0, 6, 64] = 1                                              # the true seed, far away, in the last word
    rng = np.random.default_rng(8)
    pf, pi = words(rng, 1, 2, 1, H, W), index_plane(1, 1, H, W)
    got_f, got_i, _ = check(hole, seed, pf, pi)
    assert (got_i[0, 0, 0, 3, 30:34] == 6 * W + 64).all()
    untouched = hole[0, 0] == 0
    assert np.array_equal(got_f[0, :, 0][:, untouched], pf[0, :, 0][:, untouched])


def test_a_pixel_set_in_both_masks_is_filled_not_used():
    H, W = 5, 64
    hole, seed = np.zeros((1, 1, H, W), np.uint8), np.zeros((1, 1, H, W), np.uint8)
    hole[0, 0, 2, 10:13] = 1
    seed[0, 0, 2, 11] = 1                                              # in both
    seed[0, 0, 0, 63] = 1
    _, got_i, _ = check(hole, seed, None, index_plane(1, 1, H, W))
    assert (got_i[0, 0, 0, 2, 10:13] == 63).all()


# ------------------------------------------------------------------------------------------------ layouts and launch shapes
@pytest.fixture(scope="module")
def random_case():
    """33 x 300, hole density 0.3, seed density 0.02, B * T = 6, Cf = 20, Ci = 1; the oracle's result is computed once."""
    rng = np.random.default_rng(9)
    B, T, H, W = 2, 3, 33, 300
    hole, seed = random_masks(rng, (B, T, H, W), 0.3, 0.02)
    pf, pi = words(rng, B, 20, T, H, W), words(rng, B, 1, T, H, W)
    pf[0, :, 0, 0, 3] = NAN_WORD                                       # a NaN with a payload, and the most negative id, at (0, 3)
    pi[0, :, 0, 0, 3] = -2 ** 31
    seed[0, 0, 0, 3], hole[0, 0, 0, 3] = 1, 0
    seed[0, 0, 0, 4], hole[0, 0, 0, 4] = 0, 1                          # (0, 4) takes them: a seed at (1, 4) would lose the tie
    want, unfilled = NF.nearest_fill(hole, seed, [pf, pi])
    for a in (hole, seed, pf, pi, unfilled, *want):
        a.setflags(write=False)
    return dict(hole=hole, seed=seed, pf=pf, pi=pi, want_f=want[0], want_i=want[1], unfilled=unfilled)


def test_random_masks_and_every_bit_pattern(random_case):
    c = random_case
    got_f, got_i, unfilled = fill(c["hole"], c["seed"], c["pf"], c["pi"])
    assert np.array_equal(got_f, c["want_f"]) and np.array_equal(got_i, c["want_i"]) and np.array_equal(unfilled, c["unfilled"])
    assert (got_f[0, :, 0, 0, 4] == NAN_WORD).all() and got_i[0, 0, 0, 0, 4] == -2 ** 31
    again = fill(c["hole"], c["seed"], c["pf"], c["pi"])               # two runs are bit-identical
    assert all(np.array_equal(a, b) for a, b in zip(again, (got_f, got_i, unfilled)))


def test_strided_views_bool_masks_and_absent_planes(random_case):
    c = random_case
    B, Cf, T, H, W = c["pf"].shape
    dev = lambda a, dt=None: torch.from_numpy(np.array(a)).to(DEV) if dt is None else torch.from_numpy(np.array(a)).view(dt).to(DEV)
    hole, seed = dev(c["hole"]).bool(), dev(c["seed"]).bool()
    junk = 0x55AA55AA
    big_f = torch.full((B + 1, Cf + 5, T + 2, H, W), junk, dtype=torch.int32, device=DEV).view(torch.float32)
    big_i = torch.full((B + 2, 3, T + 1, H, W), junk, dtype=torch.int32, device=DEV)
    vf, vi = big_f[1:, 2:2 + Cf, 1:1 + T], big_i[:B, 1:2, 1:]
    assert not vf.is_contiguous() and not vi.is_contiguous()
    vf.copy_(dev(c["pf"], torch.float32))
    vi.copy_(dev(c["pi"]))
    unfilled = ops.nearest_fill(hole, seed, vf, vi)
    assert np.array_equal(vf.contiguous().view(torch.int32).cpu().numpy(), c["want_f"])
    assert np.array_equal(vi.cpu().numpy(), c["want_i"]) and np.array_equal(unfilled.cpu().numpy(), c["unfilled"])
    for big, view in ((big_f.view(torch.int32), vf.view(torch.int32)), (big_i, vi)):      # nothing outside the views was written
        assert int((big == junk).sum()) == big.numel() - view.numel()
    # Cf = 0 and Ci = 0, as None and as zero channels
    pf, pi = dev(c["pf"], torch.float32), dev(c["pi"])
    ops.nearest_fill(hole, seed, pf, None)
    ops.nearest_fill(hole, seed, pf[:, :0], pi)
    assert np.array_equal(pf.view(torch.int32).cpu().numpy(), c["want_f"]) and np.array_equal(pi.cpu().numpy(), c["want_i"])
    pf2, pi2 = dev(c["pf"], torch.float32), dev(c["pi"])
    ops.nearest_fill(hole, seed, None, pi2)
    ops.nearest_fill(hole, seed, pf2, pi2[:, :0])
    assert np.array_equal(pf2.view(torch.int32).cpu().numpy(), c["want_f"]) and np.array_equal(pi2.cpu().numpy(), c["want_i"])
    # [B,H,W] masks are T = 1
    one = dev(c["pi"])[:, :, :1].contiguous()
    u = ops.nearest_fill(hole[:, 0], seed[:, 0], None, one)
    assert u.shape == (B, 1) and np.array_equal(one.cpu().numpy(), c["want_i"][:, :, :1])
    with pytest.raises(ValueError):
        ops.nearest_fill(hole, seed, None, None)
    with pytest.raises(ValueError):
        ops.nearest_fill(hole, seed, pf[..., :150], None)


def test_more_frames_than_a_capped_launch_has_workgroups():
    B, T, H, W = 60, 5, 4, 64
    rng = np.random.default_rng(10)
    hole, seed = random_masks(rng, (B, T, H, W), 0.3, 0.02)
    pf, pi = words(rng, B, 1, T, H, W), index_plane(B, T, H, W)
    got_f, got_i, unfilled = check(hole, seed, pf, pi)
    assert (unfilled > 0).any() and (unfilled == 0).any()              # some of the 300 frames drew no seed
    # the same frames 15 times over: 18000 rows of one word each, more waves than the capped grid (4096 workgroups of 4) holds
    rep = lambda a: np.concatenate([a] * 15, 0)
    big_f, big_i, big_unfilled = fill(rep(hole), rep(seed), rep(pf), rep(pi))
    assert np.array_equal(big_f, rep(got_f)) and np.array_equal(big_i, rep(got_i)) and np.array_equal(big_unfilled, rep(unfilled))


# ------------------------------------------------------------------------------------------------ end to end, without a model
def _scene():
    """A disc (a car, id 13001) over two stuff classes (1 above row 16, 2 below), moved right by 8 px in frame 0 and by 14 px in
    frame 1 -> (out dict with dense_motion_bw / occlusion_bw, bg, fg, inst of the input frame, truth ids [1,2,H,W])."""
    H, W, T = 32, 48, 2
    yy, xx = np.mgrid[:H, :W]
    disc = lambda s: (yy - 16) ** 2 + (xx - 14 - s) ** 2 <= 36
    ground = np.where(yy < 16, 1, 2).astype(np.int32)
    ids = np.where(disc(0), 13001, ground).astype(np.int32)
    sem = np.zeros((20, H, W), np.float32)
    cls = np.where(ids >= 1000, ids // 1000, ids)
    sem[cls, yy, xx] = 1.0
    flow, occ, truth = np.zeros((1, 2, T, H, W)), np.ones((1, 1, T, H, W), np.float32), np.zeros((1, T, H, W), np.int32)
    gx, gy = np.linspace(-1, 1, W), np.linspace(-1, 1, H)
    for t, s in enumerate((8, 14)):
        ix = np.where(disc(s), xx - s, xx).astype(np.float64)          # the source pixel, then the coordinate rule inverted
        flow[0, 0, t] = ((2 * ix + 1) / W - 1 - gx[None]) * ((W - 1) / 2)
        flow[0, 1, t] = ((2 * yy + 1) / H - 1 - gy[:, None]) * ((H - 1) / 2)
        occ[0, 0, t][disc(0) & ~disc(s)] = 0.0                         # what the disc uncovered
        truth[0, t] = np.where(disc(s), 13001, ground)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    out = dict(dense_motion_bw=dev(flow.astype(np.float32)), occlusion_bw=dev(occ))
    sem = dev(sem)[None, :, None]
    return out, sem[:, :11], sem[:, 11:], dev(ids)[None, None, None], dev(truth)


def test_propagate_maps_fills_the_disocclusions():
    out, bg, fg, inst, truth = _scene()
    plain = I.propagate_maps(out, bg, fg, inst, 1, occ_threshold=0.5)
    maps = I.propagate_maps(out, bg, fg, inst, 1, occ_threshold=0.5, fill="nearest")
    assert "unfilled" not in plain and not maps["unfilled"].any() and maps["unfilled"].shape == (1, 2)
    # the oracle applied to label_warp's output
    of, oi = ops.label_warp(out["dense_motion_bw"], torch.cat([bg, fg], 1)[:, :, 0], inst[:, :, 0], out["occlusion_bw"], 0.5, 0)
    assert torch.equal(oi, plain["instance_mask"])
    hole = (out["occlusion_bw"][:, 0] < 0.5).cpu().numpy()
    ids = oi[:, 0].cpu().numpy()
    seed = ~hole & ((ids < 1000) | (ids >= 19000))
    assert hole.sum() > 100 and (ids[hole] == 0).all()                 # fill_id on the holes; label_warp left "car" channels there
    assert (of[:, 13].cpu().numpy()[hole] == 1).all()
    (want_f, want_i), _ = NF.nearest_fill(hole, seed, [of.cpu().numpy(), oi.cpu().numpy()])
    got_f = torch.cat([maps["bg_mask"], maps["fg_mask"]], 1).contiguous().view(torch.int32).cpu().numpy()
    got_i = maps["instance_mask"].cpu().numpy()
    assert np.array_equal(got_f, want_f) and np.array_equal(got_i, want_i)
    # every filled pixel's one-hot class agrees with its id, and it is a background pixel now
    filled = got_i[:, 0][hole]
    onehot = got_f.view(np.float32).transpose(0, 2, 3, 4, 1)[hole]      # [n, 20]
    assert np.isin(filled, (1, 2)).all()
    assert (onehot.sum(1) == 1).all() and (onehot.argmax(1) == filled).all()
    # scored against the painted truth: strictly more correct pixels than without the fill
    correct = lambda m: int(torch.diagonal(evaluate.map_quality(m["instance_mask"], truth)["confusion"], dim1=-2, dim2=-1)[..., :19].sum())
    assert correct(maps) > correct(plain)
