"""Plain numpy / Python restatement of ops.connected_components and segment.semantic_instances, one image at a
time, written from the contract and not from the kernels: an explicit flood fill in raster order, then the ordered numbering.
No scipy here (the GPU tests import this file); tests/test_components_cpu.py holds the flood fill to scipy.ndimage.label where
scipy is installed.  cases() are the inputs the CPU and GPU tests share."""
import numpy as np

CITYSCAPES_INSTANCES = dict(thing_list=(11, 12, 13, 14, 15, 16, 17, 18), label_divisor=1000, ignore_label=255, connectivity=8,
                            min_area=1)
TILE_H, TILE_W = 16, 64             # the tile of csrc/components.hip: the cases sit on and around its seams

_NEIGHBOURS = {4: ((-1, 0), (0, -1), (0, 1), (1, 0)),
               8: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}


def connected_components(keys, connectivity=8):
    """keys [H,W] -> int32 [H,W]: at every pixel the index y * W + x of the first pixel, in raster order, of its component
    (equal key, 4- or 8-neighbours).  Pixels are visited in raster order, so the seed of a fill is the component's first pixel."""
    keys = np.asarray(keys)
    H, W = keys.shape
    nb = _NEIGHBOURS[connectivity]
    k = keys.tolist()
    out = [[-1] * W for _ in range(H)]
    for y0 in range(H):
        for x0 in range(W):
            if out[y0][x0] >= 0:
                continue
            key, seed = k[y0][x0], y0 * W + x0
            out[y0][x0] = seed
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for dy, dx in nb:
                    v, u = y + dy, x + dx
                    if 0 <= v < H and 0 <= u < W and out[v][u] < 0 and k[v][u] == key:
                        out[v][u] = seed
                        stack.append((v, u))
    return np.asarray(out, np.int32).reshape(H, W)


def components_batch(keys, connectivity=8):
    return np.stack([connected_components(k, connectivity) for k in keys]) if len(keys) else np.zeros(keys.shape, np.int32)


def semantic_instances(labels, thing_list, label_divisor, ignore_label, connectivity=8, min_area=1):
    """labels [H,W] with values 0..255 -> dict(instance int32 [H,W], count, dropped int32 [len(thing_list)], components)."""
    labels = np.asarray(labels).astype(np.int64)
    H, W = labels.shape
    comp = connected_components(labels, connectivity)
    flat_l, flat_c = labels.reshape(-1), comp.reshape(-1)
    area = np.bincount(flat_c, minlength=H * W)
    inst = labels.copy().reshape(-1)            # stuff, ignore_label, small or capped things: the label
    count = np.zeros(len(thing_list), np.int32)
    dropped = np.zeros(len(thing_list), np.int32)
    value = {}
    for root in np.flatnonzero(flat_c == np.arange(H * W)).tolist():        # roots, ascending first raster pixel
        cls = int(flat_l[root])
        if cls not in thing_list or area[root] < min_area:
            continue
        t = thing_list.index(cls)
        if count[t] < label_divisor - 1:
            count[t] += 1
            value[root] = cls * label_divisor + int(count[t])
        else:
            dropped[t] += 1
    for root, v in value.items():
        inst[flat_c == root] = v
    assert ignore_label not in thing_list
    return dict(instance=inst.reshape(H, W).astype(np.int32), count=count, dropped=dropped, components=comp)


def instances_batch(labels, **params):
    params = {**CITYSCAPES_INSTANCES, **params}
    if len(labels) == 0:
        maps, table = np.zeros(np.shape(labels), np.int32), np.zeros((0, len(params["thing_list"])), np.int32)
        return dict(instance=maps, count=table, dropped=table, components=maps)
    per = [semantic_instances(l, **params) for l in labels]
    return {k: np.stack([p[k] for p in per]) for k in ("instance", "count", "dropped", "components")}


def same_partition(a, b):
    """Do two label images split the pixels into the same sets (whatever the numbers are)?"""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    pairs = np.unique(np.stack([a, b]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))


# ------------------------------------------------------------------------------------------------ the cases
def blobs(h, w, values, cell, noise, seed):
    """A coarse random grid of `values` enlarged by `cell`, with a share `noise` of single pixels redrawn: a few large blobs at
    noise 0 and cell 8..16, thousands of specks at cell 1."""
    rng = np.random.default_rng(seed)
    values = np.asarray(values, np.uint8)
    coarse = rng.integers(0, len(values), (-(-h // cell), -(-w // cell)))
    img = np.kron(coarse, np.ones((cell, cell), np.int64))[:h, :w]
    redraw = rng.random((h, w)) < noise
    img[redraw] = rng.integers(0, len(values), int(redraw.sum()))
    return values[img]


def serpentine(h, w, path=11, rest=7):
    """A one-pixel path along the full width of every second row, joined alternately at the right and at the left end."""
    img = np.full((h, w), rest, np.uint8)
    img[0::2] = path
    for i, y in enumerate(range(1, h - 1, 2)):
        img[y, w - 1 if i % 2 == 0 else 0] = path
    return img


def spiral(n, path=13, rest=8):
    """A one-pixel square spiral from the top-left corner inwards, its arms one pixel apart."""
    g = np.zeros((n, n), bool)
    y = x = 0
    dy, dx = 0, 1
    g[0, 0] = True
    inside = lambda v, u: 0 <= v < n and 0 <= u < n
    while True:
        steps = 0
        while True:
            v, u, v2, u2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if not inside(v, u) or g[v, u] or (inside(v2, u2) and g[v2, u2]):
                break
            y, x = v, u
            g[y, x] = True
            steps += 1
        if steps == 0:
            break
        dy, dx = dx, -dy
    return np.where(g, path, rest).astype(np.uint8)


def combs(h, w, a=11, b=12, rest=0):
    """Two combs with different keys, one hanging from the top row and one standing on the bottom row, teeth interleaved."""
    img = np.full((h, w), rest, np.uint8)
    img[0, :] = a
    img[h - 1, :] = b
    img[0:h - 2, 0::4] = a
    img[2:h, 2::4] = b
    return img


def checkerboard(h, w, a=13, b=7):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where((yy + xx) % 2 == 0, a, b).astype(np.uint8)


def diagonal_contact(main):
    """Two pixels of key 11 that touch only diagonally, exactly at the corner where four tiles meet (32 x 128: 2 x 2 tiles)."""
    img = np.full((2 * TILE_H, 2 * TILE_W), 7, np.uint8)
    y, x = TILE_H - 1, TILE_W - 1
    if main:
        img[y, x] = img[y + 1, x + 1] = 11
    else:
        img[y, x + 1] = img[y + 1, x] = 11
    return img


def semantic_mix():
    """48 x 100, min_area 6: things 11, 12, 13 among stuff 0, 7, 8 and ignore_label 255."""
    img = np.zeros((48, 100), np.uint8)
    img[:, 50:] = 8
    img[2:12, 3:30] = 11                      # one car ... cut in two by an ignore stripe
    img[0:14, 15:17] = 255
    img[20:30, 5:20] = 12                     # two riders with a stuff stripe between them
    img[20:30, 12:14] = 7
    img[14:15, 40:45] = 13                    # 5 pixels: below min_area
    img[17:19, 40:43] = 13                    # 6 pixels: at min_area
    # a U of class 13 around a bar of the same class that begins ABOVE it: the enclosed one is first in raster order
    img[30:44, 60:62] = 13
    img[30:44, 78:80] = 13
    img[42:44, 60:80] = 13
    img[26:38, 69:71] = 13
    img[34:40, 86:96] = 11                    # across a tile seam (x = 64 lies in the U, y = 32 in both)
    img[40:46, 90:100] = 12                   # touches the car above: another class, another component
    img[46:48, 0:100:7] = 255
    return img


def other_classes():
    """thing_list (3, 200, 1) in that order, label_divisor 256, ignore_label 0."""
    img = blobs(37, 70, (0, 1, 3, 9, 200), 6, 0.02, 41)
    img[10:20, 60:70] = 200
    return img


def cases():
    """name -> dict(keys uint8 [N,H,W], params: keyword parameters of semantic_instances (the rest defaults to Cityscapes))."""
    c = {}
    two, three, five = (11, 7), (11, 13, 7), (0, 7, 11, 13, 255)
    for i, (h, w) in enumerate([(1, 1), (1, 70), (70, 1), (33, 65), (37, 70), (64, 128), (97, 131),
                                (TILE_H - 1, TILE_W - 1), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1),
                                (TILE_H - 1, TILE_W + 1), (TILE_H + 1, TILE_W - 1)]):
        c[f"random_{h}x{w}"] = dict(keys=np.stack([blobs(h, w, three, 1, 0.0, 10 + i),        # specks
                                                   blobs(h, w, two, 8, 0.03, 20 + i),         # blobs with some noise
                                                   blobs(h, w, five, 16, 0.0, 30 + i)]),      # a few large blobs
                                    params={})
    c["serpentine_65x67"] = dict(keys=serpentine(65, 67)[None], params={})
    c["serpentine_67x65_transposed"] = dict(keys=np.ascontiguousarray(serpentine(65, 67).T)[None], params={})
    c["spiral_67x67"] = dict(keys=spiral(67)[None], params={})
    c["combs_40x70"] = dict(keys=combs(40, 70)[None], params={})
    c["checkerboard_40x40"] = dict(keys=checkerboard(40, 40)[None], params=dict(thing_list=(13,), connectivity=4))
    # 1600 single pixels of the one thing class under 4-connectivity: the cap of label_divisor - 1 = 999 leaves 601 out
    c["checkerboard_cap_40x80"] = dict(keys=checkerboard(40, 80)[None], params=dict(thing_list=(13,), connectivity=4))
    c["diagonal_main"] = dict(keys=diagonal_contact(True)[None], params={})
    c["diagonal_anti"] = dict(keys=diagonal_contact(False)[None], params={})
    c["constant_37x70"] = dict(keys=np.full((1, 37, 70), 11, np.uint8), params={})
    c["all_ignore_33x65"] = dict(keys=np.full((1, 33, 65), 255, np.uint8), params={})
    c["semantic_mix"] = dict(keys=semantic_mix()[None], params=dict(min_area=6))
    c["semantic_mix_conn4"] = dict(keys=semantic_mix()[None], params=dict(min_area=6, connectivity=4))
    c["other_classes"] = dict(keys=other_classes()[None],
                              params=dict(thing_list=(3, 200, 1), label_divisor=256, ignore_label=0, min_area=3))
    return c
