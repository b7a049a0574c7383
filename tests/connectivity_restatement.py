"""Two independent CPU restatements of the SLIC connectivity pass (include/dcmt.h: dcmt_slic_connectivity_dev), and the planes the
tests run them and the device on.

sequential(labels, n_centers)   the reference's scan, statement by statement (DC_lidar_camera/slic.cpp:186-247): column outer, row
                                inner, a flood fill from every pixel not yet labelled, `adjlabel` carried from one component to the
                                next as there, the seed left unmarked and so counted twice.  Two departures, both dcmt.h's: the flood
                                fill's y is bounded by the rows (:226 bounds it by the columns), and the result is returned.
components(labels, n_centers)   the data-parallel definition of dcmt.h over scipy.ndimage.label: components, seeds, counts, ranks of
                                the non-small ones, links of the small ones.
Both take int32 [rows][cols] and return (int32 [rows][cols], count)."""
import numpy as np
from scipy import ndimage

DX4 = (-1, 0, 1, 0)
DY4 = (0, -1, 0, 1)


def lims_of(rows, cols, n_centers):
    return (rows * cols) // n_centers


def max_labels(rows, cols, n_centers):
    return max(1, (rows * cols) // ((lims_of(rows, cols, n_centers) >> 2) + 1))


def sequential(labels, n_centers):
    labels = np.asarray(labels)
    rows, cols = labels.shape
    lims = lims_of(rows, cols, n_centers)
    assert lims >= 4
    clusters = labels.tolist()                               # [y][x]
    new = [[-1] * cols for _ in range(rows)]
    label, adjlabel = 0, 0
    for i in range(cols):
        for j in range(rows):
            if new[j][i] != -1:
                continue
            elements = [(i, j)]
            for k in range(4):
                x, y = i + DX4[k], j + DY4[k]
                if 0 <= x < cols and 0 <= y < rows and new[y][x] >= 0:
                    adjlabel = new[y][x]
            count, c = 1, 0
            while c < count:
                ex, ey = elements[c]
                for k in range(4):
                    x, y = ex + DX4[k], ey + DY4[k]
                    if 0 <= x < cols and 0 <= y < rows and new[y][x] == -1 and clusters[j][i] == clusters[y][x]:
                        elements.append((x, y))
                        new[y][x] = label
                        count += 1
                c += 1
            if count <= lims >> 2:
                for x, y in elements:
                    new[y][x] = adjlabel
                label -= 1
            label += 1
    return np.array(new, np.int32), label


def component_ids(labels):
    """int64 [rows][cols]: the 4-connected components of equal label, numbered from 0 in no particular order."""
    ids = np.zeros(labels.shape, np.int64)
    base = 0
    for v in np.unique(labels):
        lab, n = ndimage.label(labels == v)                  # the default structure: 4-connectivity
        ids[lab > 0] = lab[lab > 0] - 1 + base
        base += n
    return ids, base


def components(labels, n_centers):
    labels = np.asarray(labels)
    rows, cols = labels.shape
    lims = lims_of(rows, cols, n_centers)
    assert lims >= 4
    ids, n = component_ids(labels)
    yy, xx = np.mgrid[0:rows, 0:cols]
    s = xx * rows + yy
    seed = np.full(n, rows * cols, np.int64)
    np.minimum.at(seed, ids.ravel(), s.ravel())
    size = np.bincount(ids.ravel(), minlength=n)
    count = size + (size >= 2)
    small = count <= lims >> 2
    final = np.full(n, -1, np.int64)
    rank = 0
    for c in np.argsort(seed):                               # every link goes to a smaller seed: its final label is known
        if not small[c]:
            final[c] = rank
            rank += 1
            continue
        x, y = divmod(int(seed[c]), rows)
        final[c] = 0
        for k in range(4):
            nx, ny = x + DX4[k], y + DY4[k]
            if 0 <= nx < cols and 0 <= ny < rows and seed[ids[ny, nx]] < seed[c]:
                final[c] = final[ids[ny, nx]]
    return final[ids].astype(np.int32), rank


def label_regions(out):
    """The number of 4-connected regions of every label of a relabelled plane: {label: regions}."""
    return {int(v): int(ndimage.label(out == v)[1]) for v in np.unique(out)}


# ------------------------------------------------------------------------------------------------------------------- the planes
def checkerboard(rows, cols):
    yy, xx = np.mgrid[0:rows, 0:cols]
    return ((xx + yy) & 1).astype(np.int32)


def h_stripes(rows, cols):
    return np.repeat((np.arange(rows, dtype=np.int32) % 3)[:, None], cols, axis=1)


def v_stripes(rows, cols):
    return np.repeat((np.arange(cols, dtype=np.int32) % 3)[None, :], rows, axis=0)


def serpentine(rows, cols):
    """A one-pixel-wide path (label 1) along every second row, joined at alternating ends; label 0 between its turns."""
    a = np.zeros((rows, cols), np.int32)
    a[0::2] = 1
    for k, y in enumerate(range(1, rows - 1, 2)):
        a[y, cols - 1 if k % 2 == 0 else 0] = 1
    return a


def comb(rows, cols):
    """A spine along the bottom row and a tooth up every second column (label 2), label 5 between the teeth."""
    a = np.full((rows, cols), 5, np.int32)
    a[rows - 1] = 2
    a[:, 0::2] = 2
    return a


def constant(rows, cols):
    return np.full((rows, cols), 3, np.int32)


def small_blocks(rows, cols):
    """2 x 3 blocks of alternating labels: many components, all of them small for n_centers = 1."""
    yy, xx = np.mgrid[0:rows, 0:cols]
    return ((yy // 2 + xx // 3) & 1).astype(np.int32) * 4


def odd_values(rows, cols, seed=5):
    """Blocky noise over -1 ("never reached"), 0, a value >= any n_centers and the two ends of int32."""
    g = np.random.Generator(np.random.PCG64(seed))
    vals = np.array([-1, 0, 7, 1 << 20, np.iinfo(np.int32).max, np.iinfo(np.int32).min], np.int32)
    coarse = g.integers(0, len(vals), ((rows + 4) // 5, (cols + 6) // 7))
    a = vals[np.kron(coarse, np.ones((5, 7), np.int64))[:rows, :cols]]
    a[g.random((rows, cols)) < 0.04] = -1
    return a.astype(np.int32)


def small_origin(rows, cols):
    """Pixel (0, 0) alone in its label; the rest in large regions."""
    a = (np.arange(cols, dtype=np.int32)[None, :] * 4 // max(cols, 1)).repeat(rows, axis=0) + 1
    a[0, 0] = 9
    return np.ascontiguousarray(a)


# name: (maker, the n_centers the tests run it with -- none below lims = 4)
PLANES = {
    "checkerboard": (checkerboard, lambda n: (1, n // 4)),
    "h_stripes": (h_stripes, lambda n: (n // 4, 3)),
    "v_stripes": (v_stripes, lambda n: (n // 4, 3)),
    "serpentine": (serpentine, lambda n: (n // 4, 2)),
    "comb": (comb, lambda n: (n // 4, 2)),
    "constant": (constant, lambda n: (1, n // 4)),
    "small_blocks": (small_blocks, lambda n: (1,)),
    "odd_values": (odd_values, lambda n: (max(1, n // 40), max(1, n // 400))),
    "small_origin": (small_origin, lambda n: (max(1, n // 16),)),
}


def plane_cases(rows, cols):
    """[(name, plane, n_centers)] of every adversarial plane at one size, n_centers capped so that lims >= 4."""
    n = rows * cols
    out = []
    for name, (make, ncs) in PLANES.items():
        for nc in sorted({max(1, min(int(c), n // 4)) for c in ncs(n)}):
            if lims_of(rows, cols, nc) >= 4:
                out.append((f"{name} {rows}x{cols} nc {nc}", make(rows, cols), nc))
    return out


def noise(rows, cols, n_values, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, n_values, (rows, cols)).astype(np.int32)
