"""Two independent statements of the speckle filter include/dcmt.h defines (dcmt_filter_speckles_dev: cv::filterSpeckles for a 16-bit
disparity map), and the inputs its tests share.

flood       the literal one: Python ints, a row-major scan as OpenCV's, a stack-based flood fill from every live pixel not yet
            labelled over the edge relation, the component's size counted as it is filled.
vectorised  numpy: every live pixel starts with its own index as label; the minimum label is propagated over the four edge masks
            until nothing changes (each label only ever falls, so the fixed point is the minimum index of the component), then
            np.bincount gives the sizes.

Both return (out int16 [rows][cols], changed bool [rows][cols]); with_depth() applies the depth rule and counts.  Nothing here is
fitted to the library: tests/test_speckle.py holds the two against each other without a GPU."""
import numpy as np

f32 = np.float32
DEFAULTS = dict(max_size=200, max_diff=32, new_val=-16)
MAX_DIFFS = (0, 15, 16, 32, 65535)


def params(**kw):
    assert set(kw) <= set(DEFAULTS), kw
    p = dict(DEFAULTS)
    p.update(kw)
    assert p["max_size"] >= 0 and 0 <= p["max_diff"] <= 65535 and -32768 <= p["new_val"] <= 32767
    return p


# ---- the statement, pixel by pixel -----------------------------------------------------------------------------------------------
def flood(disp16, **kw):
    p = params(**kw)
    max_size, max_diff, new_val = p["max_size"], p["max_diff"], p["new_val"]
    assert disp16.dtype == np.int16 and disp16.ndim == 2
    rows, cols = disp16.shape
    v = disp16.astype(int).tolist()
    seen = [[False] * cols for _ in range(rows)]
    changed = np.zeros((rows, cols), bool)
    for y in range(rows):
        for x in range(cols):
            if seen[y][x] or v[y][x] == new_val:
                continue
            seen[y][x] = True
            stack, members = [(y, x)], []
            while stack:
                cy, cx = stack.pop()
                members.append((cy, cx))
                for ny, nx in ((cy, cx + 1), (cy, cx - 1), (cy + 1, cx), (cy - 1, cx)):
                    if 0 <= ny < rows and 0 <= nx < cols and not seen[ny][nx] and v[ny][nx] != new_val and \
                            abs(v[ny][nx] - v[cy][cx]) <= max_diff:           # Python ints: -32768 against 32767 is 65535
                        seen[ny][nx] = True
                        stack.append((ny, nx))
            if len(members) <= max_size:
                for my, mx in members:
                    changed[my, mx] = True
    out = disp16.copy()
    out[changed] = new_val
    return out, changed


# ---- the same, planes at a time -----------------------------------------------------------------------------------------------------
def components(disp16, max_diff, new_val):
    """(label int64 [rows][cols]: the smallest row-major index of the pixel's component, -1 on dead pixels; size of each pixel's
    component, 0 on dead pixels)."""
    rows, cols = disp16.shape
    v = disp16.astype(np.int64)
    live = v != new_val
    right = live[:, :-1] & live[:, 1:] & (np.abs(v[:, :-1] - v[:, 1:]) <= max_diff)          # edge (y, x) - (y, x + 1)
    down = live[:-1, :] & live[1:, :] & (np.abs(v[:-1, :] - v[1:, :]) <= max_diff)           # edge (y, x) - (y + 1, x)
    big = rows * cols
    label = np.where(live, np.arange(big).reshape(rows, cols), big)
    while True:
        new = label.copy()
        np.minimum(new[:, 1:], np.where(right, label[:, :-1], big), out=new[:, 1:])
        np.minimum(new[:, :-1], np.where(right, label[:, 1:], big), out=new[:, :-1])
        np.minimum(new[1:, :], np.where(down, label[:-1, :], big), out=new[1:, :])
        np.minimum(new[:-1, :], np.where(down, label[1:, :], big), out=new[:-1, :])
        # a label is a pixel index: jump to that pixel's label too, which halves the chains a serpentine makes
        flat = np.append(new.ravel(), big)
        new = np.minimum(new, flat[new])
        if np.array_equal(new, label):
            break
        label = new
    counts = np.bincount(label.ravel(), minlength=big + 1)
    size = np.where(live, counts[label], 0)
    return np.where(live, label, -1), size


def vectorised(disp16, **kw):
    p = params(**kw)
    assert disp16.dtype == np.int16 and disp16.ndim == 2
    _, size = components(disp16, p["max_diff"], p["new_val"])
    changed = (size > 0) & (size <= p["max_size"])
    out = disp16.copy()
    out[changed] = p["new_val"]
    return out, changed


def with_depth(fn, disp16, depth=None, **kw):
    """(out, depth' or None, removed): the depth plane keeps its bits except +0.0 where the call changed the disparity."""
    out, changed = fn(disp16, **kw)
    z = None
    if depth is not None:
        z = depth.copy()
        z.view(np.uint32)[changed] = 0
    return out, z, int(changed.sum())


def batch(fn, planes, depths=None, **kw):
    outs = [with_depth(fn, d, None if depths is None else depths[i], **kw) for i, d in enumerate(planes)]
    return (np.stack([o[0] for o in outs]), None if depths is None else np.stack([o[1] for o in outs]),
            np.array([o[2] for o in outs], np.uint32))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def random_plane(rows, cols, k, live, seed, new_val=-16):
    """Values from {0, 16, ..., 16 k}, a fraction `live` of the pixels; the others new_val."""
    rng = np.random.default_rng(seed)
    v = (16 * rng.integers(0, k + 1, (rows, cols))).astype(np.int16)
    v[rng.random((rows, cols)) >= live] = new_val
    return v


def depth_pattern(shape, seed=0):
    """An f32 plane with a bit pattern of its own in every pixel (NaNs, infinities and -0 among them): "untouched" is checked on bits."""
    n = int(np.prod(shape))
    bits = (np.arange(n, dtype=np.uint64) * 2654435761 + 0x9e3779b9 * (seed + 1)) % (1 << 32)
    bits = bits.astype(np.uint32)
    bits[bits == 0] = 0x80000000                   # +0.0 is what a removed pixel gets: keep it out of the pattern
    return bits.view(f32).reshape(shape)


BLOCK = np.array([[-32, 32], [0, 0]], np.int16)          # at max_diff 32: one component of 4 whose top pair is no edge


def block_plane(rows, cols, y, x, rot, new_val=-16):
    """The 2 x 2 block, rotated rot quarter turns, with its top-left pixel at (y, x) of an otherwise dead plane."""
    v = np.full((rows, cols), new_val, np.int16)
    v[y:y + 2, x:x + 2] = np.rot90(BLOCK, rot)
    return v


def ramp(rows, cols, step):
    v = step * (np.arange(rows)[:, None] + np.arange(cols)[None, :])
    assert v.max() <= 32767
    return v.astype(np.int16)


def serpentine(rows, cols, length, value=100, new_val=-16):
    """A one-pixel-wide path of exactly `length` live pixels: along even rows 0, 2, 4, ... alternately rightwards and leftwards,
    joined by one pixel in the odd row between, at the end the row turned at."""
    v = np.full((rows, cols), new_val, np.int16)
    path = []
    for y in range(0, rows, 2):
        xs = range(cols) if (y // 2) % 2 == 0 else range(cols - 1, -1, -1)
        path += [(y, x) for x in xs]
        if y + 2 < rows:
            path.append((y + 1, path[-1][1]))
    assert 1 <= length <= len(path), (length, len(path))
    for y, x in path[:length]:
        v[y, x] = value
    return v


def stamp_blobs(disp16, count, seed, offset=200):
    """`count` blobs of at most 9 pixels (3 x 3 with random pixels left out, never the centre), each at a value `offset` sixteenths
    above the largest value of the plane around it (so further than 32 from everything), at least 4 pixels apart from each other and
    from the frame's edge.  Returns (stamped plane, mask of the stamped pixels)."""
    rng = np.random.default_rng(seed)
    rows, cols = disp16.shape
    out, mask = disp16.copy(), np.zeros(disp16.shape, bool)
    centres = []
    while len(centres) < count:
        y, x = int(rng.integers(4, rows - 4)), int(rng.integers(4, cols - 4))
        if all(max(abs(y - cy), abs(x - cx)) >= 6 for cy, cx in centres):
            centres.append((y, x))
    for i, (y, x) in enumerate(centres):
        keep = rng.random((3, 3)) < 0.7
        keep[1, 1] = True
        # a value of its own per blob, far from the plane's (<= 16 * 127 + 8) and from the other blobs'
        value = int(disp16.max()) + offset * (i + 1)
        assert value <= 32767
        blob = np.zeros(disp16.shape, bool)
        blob[y - 1:y + 2, x - 1:x + 2] = keep
        out[blob] = value
        mask |= blob
    return out, mask
