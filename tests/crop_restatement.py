"""dcmt_crop_frames_dev and dcmt_depth_to_u16* restated in numpy: what tests/test_crop.py pins on a CPU and what
tests/test_gpu_crop_export.py compares the device bytes with.  Nothing here calls the library."""
import numpy as np

KITTI_SIZES = [(375, 1242), (370, 1224), (374, 1238), (370, 1226), (376, 1241)]      # the five recording days
KITTI_ORIGINS = [(23, 13), (18, 4), (22, 11), (18, 5), (24, 12)]                      # (y0, x0) of the bottom-centre 352 x 1216 window
EXPORT_PROBES = [0.0, -1.5, 0.5 / 256, 1.5 / 256, 2.5 / 256, 65535 / 256, 256.0, 1e30, -0.0]
EXPORT_WANT = [0, 0, 0, 2, 2, 65535, 65535, 65535, 0]


def depth_to_u16(x, scale=256.0) -> np.ndarray:
    """clip(rint(f32(x) * f32(scale)), 0, 65535): one f32 rounding in the product, ties to even, saturated (an overflow to +Inf
    included)."""
    with np.errstate(over="ignore"):
        t = np.asarray(x, dtype=np.float32) * np.float32(scale)
    assert t.dtype == np.float32
    return np.clip(np.rint(t), 0, 65535).astype(np.uint16)


def record_ok(rec, elem: int, out_rows: int, out_cols: int, src_bytes: int) -> bool:
    """The record test of include/dcmt.h in Python's unbounded integers."""
    off, st, rows, cols, x0, y0 = (int(rec[k]) for k in ("offset", "row_stride", "rows", "cols", "x0", "y0"))
    return (rows >= 1 and cols >= 1 and x0 >= 0 and y0 >= 0 and x0 + out_cols <= cols and y0 + out_rows <= rows and st >= cols * elem
            and off <= src_bytes and (rows - 1) * st + cols * elem <= src_bytes - off)


def crop_frames(buf, table, elem: int, out_rows: int, out_cols: int, src_bytes=None) -> np.ndarray:
    """uint8 [batch][out_rows][out_cols * elem]: per frame the window's bytes, numpy slicing on a strided view of the source bytes;
    zeros where the record is bad."""
    buf = np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
    src_bytes = len(buf) if src_bytes is None else src_bytes
    out = np.zeros((len(table), out_rows, out_cols * elem), np.uint8)
    for f, rec in enumerate(table):
        if not record_ok(rec, elem, out_rows, out_cols, src_bytes):
            continue
        off, st, rows, cols = int(rec["offset"]), int(rec["row_stride"]), int(rec["rows"]), int(rec["cols"])
        frame = np.lib.stride_tricks.as_strided(buf[off:], shape=(rows, cols * elem), strides=(st, 1), writeable=False)
        x0, y0 = int(rec["x0"]), int(rec["y0"])
        out[f] = frame[y0:y0 + out_rows, x0 * elem:(x0 + out_cols) * elem]
    return out


def noise(shape, dtype, seed) -> np.ndarray:
    """Every byte random, none of the values special."""
    g = np.random.Generator(np.random.PCG64(seed))
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return g.integers(0, 256, n, dtype=np.uint8).view(dtype).reshape(shape)
