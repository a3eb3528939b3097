"""csrc/resize.hip vs the NumPy restatements of tests/resize_np.py (pinned to Pillow and torch by test_resize_cpu.py): frames and
maps bit for bit, flows within the fp32 rounding bound of two dot products."""
import functools

import numpy as np
import pytest
import torch

import resize_np as R
from c2m_amd import data

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 3
# output 37 x 70: three 16-row and three 32-column tiles, neither a multiple of the tile
CASES = R.SHAPES + [((75, 150), (37, 70))]


@functools.lru_cache(maxsize=None)
def _inputs(shape_in, C):
    return R.patterns(np.random.default_rng(hash((shape_in, C)) % 2 ** 32), (N,) + shape_in + (C,))


@functools.lru_cache(maxsize=None)
def _want(shape_in, size, C, name, filt):
    return R.np_resize_u8(_inputs(shape_in, C)[name], size, filt)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("shape_in,size", CASES)
def test_bicubic_equals_pillow_restatement(shape_in, size, C):
    for name, img in _inputs(shape_in, C).items():
        got = data.resize_frames(torch.from_numpy(img).to(DEV), size)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (N,) + size + (C,)
        want = torch.from_numpy(_want(shape_in, size, C, name, "bicubic"))
        assert torch.equal(got.cpu(), want), f"{name}: {int((got.cpu() != want).sum())} of {want.numel()} values differ"


@pytest.mark.parametrize("shape_in,size", [CASES[0], CASES[2], CASES[4]])
def test_bilinear_equals_pillow_restatement(shape_in, size):
    img = _inputs(shape_in, 3)["noise"]
    got = data.resize_frames(torch.from_numpy(img).to(DEV), size, filter="bilinear")
    assert torch.equal(got.cpu(), torch.from_numpy(_want(shape_in, size, 3, "noise", "bilinear")))


def test_frames_with_leading_dims_and_unaligned_storage():
    """[B,T,H,W,3] as assemble_batch passes it, and a view whose first byte is not dword aligned (rows are fetched as dwords)."""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (2, 2, 37, 53, 3), dtype=np.uint8)
    want = torch.from_numpy(R.np_resize_u8(img, (16, 24)))
    assert torch.equal(data.resize_frames(torch.from_numpy(img).to(DEV), (16, 24)).cpu(), want)
    flat = torch.zeros(img.size + 1, dtype=torch.uint8, device=DEV)
    flat[1:] = torch.from_numpy(img.reshape(-1)).to(DEV)
    view = flat[1:].view(2, 2, 37, 53, 3)
    assert view.data_ptr() % 4 == 1 and view.is_contiguous()
    assert torch.equal(data.resize_frames(view, (16, 24)).cpu(), want)


def test_full_size_frame():
    img = np.random.default_rng(9).integers(0, 256, (1, 1024, 2048, 3), dtype=np.uint8)
    got = data.resize_frames(torch.from_numpy(img).to(DEV), (128, 256))
    assert torch.equal(got.cpu(), torch.from_numpy(R.np_resize_u8(img, (128, 256))))


@pytest.mark.parametrize("shape_in,size", CASES + [((1024, 2048), (128, 256))])
def test_nearest_equals_pillow_restatement(shape_in, size):
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 40001, (N,) + shape_in).astype(np.int32)
    ids[0, 0, 0], ids[0, -1, -1] = 40000, 40000
    for x in (ids, (ids % 256).astype(np.uint8)):
        got = data.resize_maps(torch.from_numpy(x).to(DEV), size)
        assert got.dtype == torch.from_numpy(x).dtype
        assert torch.equal(got.cpu(), torch.from_numpy(R.np_resize_nearest(x, size)))


def _flow_bound(shape_in, size, antialias, flow):
    """8 * n_taps * 2^-24 * max|v|: two fp32 dot products of n non-negative weights summing to 1, plus the fp32 cast of the
    weights."""
    return 8 * R.flow_max_taps(shape_in, size, antialias) * 2.0 ** -24 * float(np.abs(flow).max())


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("shape_in,size", CASES)
def test_flow_within_rounding_of_float64(shape_in, size, antialias):
    flow = (np.random.default_rng(7).standard_normal((N,) + shape_in + (2,)) * 6.0).astype(np.float32)
    got = data.resize_flow(torch.from_numpy(flow).to(DEV), size, antialias=antialias).cpu().numpy()
    want = R.np_resize_flow(flow, size, antialias)
    err, bound = float(np.abs(got - want).max()), _flow_bound(shape_in, size, antialias, flow)
    print(f"flow {shape_in}->{size} antialias={antialias}: max error {err:.3e}, bound {bound:.3e}")
    assert got.shape == want.shape and err <= bound
    ones = np.ones((1,) + shape_in + (2,), np.float32)                      # the Hout / Hin factor, on both channels
    got1 = data.resize_flow(torch.from_numpy(ones).to(DEV), size, antialias=antialias).cpu().numpy()
    assert np.abs(got1 - size[0] / shape_in[0]).max() <= _flow_bound(shape_in, size, antialias, ones)


def test_assemble_batch_resizes_on_the_device():
    B, T, H, W, size = 2, 3, 64, 128, (32, 64)
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (B, T, H, W, 3), dtype=np.uint8)
    labels = rng.integers(0, 34, (B, T, H, W), dtype=np.uint8)
    inst = rng.integers(0, 40001, (B, T, H, W)).astype(np.int32)
    occ = (rng.integers(0, 2, (B, T, H, W)) * 255).astype(np.uint8)
    flow = (rng.standard_normal((B, T, H, W, 2)) * 4.0).astype(np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    for antialias in (False, True):
        got = data.assemble_batch(dev(frames), dev(labels), dev(inst), dev(occ[:, 1:]), dev(flow[:, 1:]), None, dev(occ[:, :1]),
                                  dev(flow[:, :1]), size=size, antialias=antialias)
        rflow = R.np_resize_flow(flow, size, antialias)
        want = data.assemble_batch(dev(R.np_resize_u8(frames, size)), dev(R.np_resize_nearest(labels, size)),
                                   dev(R.np_resize_nearest(inst, size)), dev(R.np_resize_nearest(occ[:, 1:], size)),
                                   dev(rflow[:, 1:].astype(np.float32)), None, dev(R.np_resize_nearest(occ[:, :1], size)),
                                   dev(rflow[:, :1].astype(np.float32)))
        for k in ("video", "bg_mask", "fg_mask", "instance_mask", "target_bw_occ", "input_occ"):
            assert torch.equal(got[k], want[k]), k
        bound = _flow_bound((H, W), size, antialias, flow)
        for k, part in (("target_bw_of", rflow[:, 1:]), ("input_of", rflow[:, :1])):
            ref = np.moveaxis(part, -1, 1)                                    # [B,T,h,w,2] float64 -> [B,2,T,h,w]
            assert got[k].shape == want[k].shape == ref.shape
            assert float(np.abs(got[k].cpu().numpy() - ref).max()) <= bound, k


def test_validation_empty_batch_and_same_size():
    u8 = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError):
        data.resize_frames(u8.cpu(), (4, 4))                                  # not on the device: no CPU path
    with pytest.raises(TypeError):
        data.resize_frames(u8.float(), (4, 4))
    with pytest.raises(TypeError):
        data.resize_maps(torch.zeros(1, 8, 8, dtype=torch.int64, device=DEV), (4, 4))
    with pytest.raises(TypeError):
        data.resize_flow(torch.zeros(1, 8, 8, 2, dtype=torch.float64, device=DEV), (4, 4))
    with pytest.raises(ValueError):
        data.resize_frames(torch.zeros(1, 8, 8, 2, dtype=torch.uint8, device=DEV), (4, 4))      # C not in {1, 3}
    with pytest.raises(ValueError):
        data.resize_frames(torch.zeros(8, 8, dtype=torch.uint8, device=DEV), (4, 4))            # rank
    with pytest.raises(ValueError):
        data.resize_maps(torch.zeros(8, dtype=torch.uint8, device=DEV), (4, 4))
    with pytest.raises(ValueError):
        data.resize_flow(torch.zeros(1, 8, 8, 3, device=DEV), (4, 4))
    with pytest.raises(ValueError):
        data.resize_frames(u8, (0, 4))
    with pytest.raises(ValueError):
        data.resize_maps(u8[..., 0], (4, -1))
    with pytest.raises(ValueError):
        data.resize_frames(u8, (4, 4), filter="lanczos")
    with pytest.raises(ValueError):
        data.resize_frames(torch.zeros(1, 0, 8, 3, dtype=torch.uint8, device=DEV), (4, 4))      # an image without rows
    assert data.resize_frames(u8[:0], (4, 6)).shape == (0, 4, 6, 3)
    assert data.resize_maps(torch.zeros(0, 5, 8, 8, dtype=torch.int32, device=DEV), (4, 6)).shape == (0, 5, 4, 6)
    assert data.resize_flow(torch.zeros(0, 8, 8, 2, device=DEV), (4, 6)).shape == (0, 4, 6, 2)
    assert data.resize_frames(u8, (8, 8)) is u8                               # already at size: returned as it is
    m = torch.zeros(2, 8, 8, dtype=torch.int32, device=DEV)
    assert data.resize_maps(m, (8, 8)) is m
