"""Two independent CPU restatements of SLIC's two pixel renderings (include/dcmt.h: dcmt_slic_contours_dev,
dcmt_slic_cluster_means_dev), and the planes the tests run them and the device on.

literal_contours(labels)        Slic::display_contours statement by statement (DC_lidar_camera/slic.cpp:337-384): column outer, row
                                inner, the istaken matrix, the eight neighbours in the order of dx8 / dy8.  Returns the uint8 mask
                                (255 where :373-374 pushes the pixel); paint() is :379-383.
closed_contours(labels)         the definition of dcmt.h, vectorised in numpy: A and the three west "differs" planes for the whole
                                frame at once, then column by column c, the constant pixels, and for every pixel the nearest
                                constant pixel at or above it with the parity of the distance (no scan down the column).
literal_means(labels, image, n) Slic::colour_with_cluster_means statement by statement (:392-433) in Python floats (doubles), the
                                count being center_counts' definition (:142-163: the pixels of the label); a label outside [0, n)
                                is skipped, as dcmt.h states.  Returns (image, sums [n][4]).
closed_means(labels, image, n)  np.bincount and integer division.
Labels are int32 [rows][cols]; images uint8 [rows][cols][3], B, G, R."""
import numpy as np

DX8 = (-1, -1, 0, 1, 1, 1, 0, -1)
DY8 = (0, -1, -1, -1, 0, 1, 1, 1)
i32 = np.int32


def literal_contours(labels):
    labels = np.asarray(labels)
    rows, cols = labels.shape
    clusters = labels.T.tolist()                             # [x][y], as Slic::clusters
    istaken = [[False] * rows for _ in range(cols)]
    contours = []
    for i in range(cols):
        for j in range(rows):
            nr_p = 0
            for k in range(8):
                x, y = i + DX8[k], j + DY8[k]
                if 0 <= x < cols and 0 <= y < rows:
                    if istaken[x][y] is False and clusters[i][j] != clusters[x][y]:
                        nr_p += 1
            if nr_p >= 2:
                contours.append((i, j))
                istaken[i][j] = True
    mask = np.zeros((rows, cols), np.uint8)
    for x, y in contours:
        mask[y, x] = 255
    return mask


def paint(image, mask, colour=(0, 0, 200)):
    out = np.array(image, dtype=np.uint8)
    out[mask != 0] = np.array(colour, np.uint8)              # (uchar)colour[0..2], :380-381
    return out


def _differs(labels, dx, dy):
    """bool [rows][cols]: (x + dx, y + dy) is inside the frame and has another label."""
    rows, cols = labels.shape
    out = np.zeros((rows, cols), bool)
    ys, yd = (slice(max(0, -dy), rows - max(0, dy)), slice(max(0, dy), rows - max(0, -dy)))
    xs, xd = (slice(max(0, -dx), cols - max(0, dx)), slice(max(0, dx), cols - max(0, -dx)))
    out[ys, xs] = labels[ys, xs] != labels[yd, xd]
    return out


def closed_terms(labels):
    """(A, west_up, west, west_down, north) of dcmt.h for every pixel."""
    labels = np.asarray(labels)
    A = sum(_differs(labels, dx, dy).astype(np.int64) for dx, dy in ((1, -1), (1, 0), (1, 1), (0, 1)))
    return A, _differs(labels, -1, -1), _differs(labels, -1, 0), _differs(labels, -1, 1), _differs(labels, 0, -1)


def closed_contours(labels, runs=None):
    """runs: a list that receives (x, first row, length) of every alternating run (maximal run of c == 1 pixels under differing upper pixels)."""
    labels = np.asarray(labels)
    rows, cols = labels.shape
    A, wu, wm, wd, north = closed_terms(labels)
    taken = np.zeros((rows, cols), bool)
    prev = np.zeros(rows + 2, bool)                          # the previous column's taken bits, one row of padding above and below
    yy = np.arange(rows)
    for x in range(cols):
        c = A[:, x] + (wu[:, x] & ~prev[0:rows]) + (wm[:, x] & ~prev[1:rows + 1]) + (wd[:, x] & ~prev[2:rows + 2])
        constant = ~north[:, x] | (c != 1)                   # row 0 is always constant: (x, -1) is outside the frame
        base = np.maximum.accumulate(np.where(constant, yy, -1))     # the nearest constant row at or above each row
        col = (c[base] >= 2) ^ (((yy - base) & 1) == 1)
        taken[:, x] = col
        prev[1:rows + 1] = col
        if runs is not None:
            start = None
            for y in range(rows + 1):
                inside = y < rows and not constant[y]
                if inside and start is None:
                    start = y
                if not inside and start is not None:
                    runs.append((x, start, y - start))
                    start = None
    return np.where(taken, 255, 0).astype(np.uint8)


def literal_means(labels, image, n_labels):
    labels, image = np.asarray(labels), np.asarray(image)
    rows, cols = labels.shape
    clusters, img = labels.T.tolist(), image.tolist()
    colours = [[0.0, 0.0, 0.0] for _ in range(n_labels)]
    center_counts = [0] * n_labels
    for i in range(cols):
        for j in range(rows):
            index = clusters[i][j]
            if not 0 <= index < n_labels:
                continue
            colour = img[j][i]
            colours[index][0] += colour[0]
            colours[index][1] += colour[1]
            colours[index][2] += colour[2]
            center_counts[index] += 1
    sums = np.array([[int(c[0]), int(c[1]), int(c[2]), n] for c, n in zip(colours, center_counts)], i32).reshape(n_labels, 4)
    for i in range(n_labels):
        if center_counts[i]:
            for ch in range(3):
                colours[i][ch] /= center_counts[i]
    out = np.array(image, dtype=np.uint8)
    for i in range(cols):
        for j in range(rows):
            index = clusters[i][j]
            if 0 <= index < n_labels:
                out[j, i] = [int(colours[index][0]), int(colours[index][1]), int(colours[index][2])]   # double -> uchar: truncation
    return out, sums


def closed_means(labels, image, n_labels):
    labels, image = np.asarray(labels), np.asarray(image)
    ok = (labels >= 0) & (labels < n_labels)
    lab = labels[ok].astype(np.int64)
    sums = np.zeros((n_labels, 4), np.int64)
    for ch in range(3):
        np.add.at(sums[:, ch], lab, image[..., ch][ok].astype(np.int64))
    np.add.at(sums[:, 3], lab, 1)
    out = np.array(image, dtype=np.uint8)
    mean = sums[:, :3] // np.maximum(sums[:, 3:], 1)
    out[ok] = mean[lab].astype(np.uint8)
    return out, sums.astype(i32)


# ---------------------------------------------------------------------------------------------------------------- the planes
def noise(rows, cols, n_values, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, n_values, (rows, cols)).astype(i32)


def rows_own_label(rows, cols):
    """Every row its own label: every column is one alternating run from row 1 down (the 130 x 3 plane's run of 127 is the last column's)."""
    return np.broadcast_to(np.arange(rows, dtype=i32)[:, None], (rows, cols)).copy()


def h_stripes(rows, cols, height=3):
    return np.broadcast_to((np.arange(rows, dtype=i32) // height)[:, None], (rows, cols)).copy()


def v_stripes(rows, cols, width=2):
    return np.broadcast_to((np.arange(cols, dtype=i32) // width)[None, :], (rows, cols)).copy()


def checkerboard(rows, cols):
    yy, xx = np.mgrid[0:rows, 0:cols]
    return ((yy + xx) & 1).astype(i32)


def constant(rows, cols):
    return np.full((rows, cols), 3, i32)


def out_of_range(rows, cols, n_labels=6, seed=5):
    """Blocks of labels of which some are -1, some >= n_labels, one INT32_MIN."""
    g = np.random.Generator(np.random.PCG64(seed))
    vals = np.array([-1, 0, 1, n_labels - 1, n_labels, n_labels + 7, np.iinfo(i32).min, 2], i32)
    small = vals[g.integers(0, len(vals), ((rows + 2) // 3, (cols + 3) // 4))]
    return np.kron(small, np.ones((3, 4), i32))[:rows, :cols].astype(i32)


def voronoi(rows, cols, n=12, seed=3):
    g = np.random.Generator(np.random.PCG64(seed))
    py, px = g.uniform(0, rows, n), g.uniform(0, cols, n)
    yy, xx = np.mgrid[0:rows, 0:cols]
    return np.argmin((yy[..., None] - py) ** 2 + (xx[..., None] - px) ** 2, axis=-1).astype(i32)


PLANES = ("rows", "hstripes", "checkerboard", "vstripes", "constant", "outofrange")


def plane_cases(rows, cols):
    """(name, plane) for every adversarial plane at this size."""
    return [(f"rows {rows}x{cols}", rows_own_label(rows, cols)), (f"hstripes {rows}x{cols}", h_stripes(rows, cols)),
            (f"checkerboard {rows}x{cols}", checkerboard(rows, cols)), (f"vstripes {rows}x{cols}", v_stripes(rows, cols)),
            (f"constant {rows}x{cols}", constant(rows, cols)), (f"outofrange {rows}x{cols}", out_of_range(rows, cols))]


def image_for(rows, cols, seed):
    return np.random.Generator(np.random.PCG64(1000 + seed)).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
