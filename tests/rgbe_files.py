"""A writer of Radiance .hdr pictures for the tests of host/rgbe.hpp: no fixture files.  float -> RGBE as Radiance's
setcolr does it, and the three scanline encodings the reader takes — flat, the old run pixels, the new run-length coded planes — with either
row order and any extra header lines."""
import numpy as np


def float_to_rgbe(rgb):
    """[H, W, 3] floats -> uint8 [H, W, 4]: v = max(r, g, b); v < 1e-32 is (0, 0, 0, 0); else v = m * 2^e with m in [0.5, 1), the channels are
    floor(c * m * 256 / v) and the exponent byte is e + 128 (color.c: setcolr)."""
    rgb = np.asarray(rgb, dtype=np.float64)
    v = rgb.max(axis=-1)
    m, e = np.frexp(v)
    live = v >= 1e-32
    k = np.where(live, m * 256.0 / np.where(live, v, 1.0), 0.0)
    out = np.zeros(rgb.shape[:-1] + (4,), dtype=np.uint8)
    out[..., :3] = np.clip(np.floor(rgb * k[..., None]), 0, 255).astype(np.uint8)
    out[..., 3] = np.where(live, e + 128, 0).astype(np.uint8)
    out[~live] = 0
    return out


def rgbe_to_float(rgbe):
    """uint8 [..., 4] -> float64 [..., 3]: e == 0 is black, else m * 2^(e - 136), with no + 0.5."""
    rgbe = np.asarray(rgbe, dtype=np.uint8)
    e = rgbe[..., 3].astype(np.int64)
    return np.where((e == 0)[..., None], 0.0, np.ldexp(rgbe[..., :3].astype(np.float64), (e - 136)[..., None]))


def header(width, height, flip=False, extra=(), fmt="32-bit_rle_rgbe", signature="#?RADIANCE", resolution=None):
    """The text header, the empty line and the resolution line.  fmt None leaves the FORMAT line out; extra: further header lines;
    resolution: the whole resolution line, for the orientations the reader refuses."""
    lines = [signature] + list(extra) + (["FORMAT=" + fmt] if fmt else []) + [""]
    lines.append(resolution if resolution is not None else "%sY %d +X %d" % ("+" if flip else "-", height, width))
    return ("\n".join(lines) + "\n").encode("ascii")


def scan_flat(row):
    """One scanline as it is: W quadruples."""
    return np.ascontiguousarray(row, dtype=np.uint8).tobytes()


def scan_old_runs(row):
    """Flat pixels where each repeat of the previous pixel within the line is folded into run pixels (1, 1, 1, n): n << 0 copies, and for a run
    of 256 or more a second, consecutive run pixel that counts n << 8 (color.c: oldreadcolrs)."""
    row = np.ascontiguousarray(row, dtype=np.uint8)
    assert not (row[:, :3] == 1).all(axis=1).any(), "a pixel (1, 1, 1, n) cannot be written flat"
    out, x, w = bytearray(), 0, row.shape[0]
    while x < w:
        out += row[x].tobytes()
        n = 1
        while x + n < w and (row[x + n] == row[x]).all():
            n += 1
        rep = n - 1
        if rep >= 256:
            out += bytes([1, 1, 1, rep & 255, 1, 1, 1, rep >> 8])
        elif rep >= 2:
            out += bytes([1, 1, 1, rep])
        elif rep == 1:
            out += row[x].tobytes()
        x += n
    return bytes(out)


def plane_rle(plane, min_run=4):
    """One channel plane of a new-style scanline: a count byte > 128 is a run of count - 128 copies of the next byte (at most 127), a count of 1..128
    that many literal bytes.  Runs shorter than min_run go into the literals."""
    plane = [int(b) for b in plane]
    out, lit, x, w = bytearray(), [], 0, len(plane)

    def flush():
        while lit:
            out.append(min(len(lit), 128))
            out.extend(lit[:128])
            del lit[:128]

    while x < w:
        n = 1
        while x + n < w and plane[x + n] == plane[x]:
            n += 1
        if n >= min_run:
            flush()
            left = n
            while left:
                k = min(left, 127)
                out += bytes([128 + k, plane[x]])
                left -= k
        else:
            lit.extend(plane[x:x + n])
        x += n
    flush()
    return bytes(out)


def scan_rle(row, min_run=4):
    """One new-style scanline: 2, 2, W >> 8, W & 255, then the four planes (8 <= W < 32768)."""
    row = np.ascontiguousarray(row, dtype=np.uint8)
    w = row.shape[0]
    assert 8 <= w < 32768
    return bytes([2, 2, w >> 8, w & 255]) + b"".join(plane_rle(row[:, ch], min_run) for ch in range(4))


ENCODERS = {"flat": scan_flat, "old": scan_old_runs, "rle": scan_rle}


def write_hdr(rgbe, encoding="rle", flip=False, **head):
    """uint8 [H, W, 4] (top-down) -> the bytes of a .hdr file.  flip writes "+Y H +X W" and the rows bottom-up."""
    rgbe = np.ascontiguousarray(rgbe, dtype=np.uint8)
    h, w = rgbe.shape[:2]
    if encoding != "rle":
        assert w < 8 or not (rgbe[:, 0, 0] == 2).any(), "a flat line that starts with 2 could be taken for a run-length coded one"
    rows = rgbe[::-1] if flip else rgbe
    return header(w, h, flip=flip, **head) + b"".join(ENCODERS[encoding](r) for r in rows)


def sample_image(width, height, seed=0):
    """uint8 [H, W, 4]: positive values over many exponents with constant stretches (runs in every plane, pixel repeats for the old runs), a ramp
    (long literals), and noise.  From float_to_rgbe, so the largest mantissa of a pixel is at least 128: no pixel is (1, 1, 1, n) or starts with 2."""
    rng = np.random.default_rng(1000 * width + height + seed)
    rgb = rng.uniform(0.01, 1.0, size=(height, width, 3)) * np.exp2(rng.integers(-6, 7, size=(height, width, 1)))
    x = np.arange(width)
    rgb[:, (x % 13) < 6] = rgb[:, :1]                                  # stretches that repeat the line's first pixel
    if width >= 128:
        rgb[:, :, 0] = 0.75                                            # a constant plane: one run of 127 and one more byte
        rgb[:, :, 1] = 0.3 + 0.002 * x                                 # a ramp: a literal of 128
        rgb[:, :, 2] = np.where(x < 40, 0.6, rgb[:, :, 2])
    out = float_to_rgbe(rgb)
    if width >= 128:
        out[..., 3] = 128                                              # one exponent, and the two planes byte for byte what their comments say
        out[:, :, 0] = 192
        out[:, :, 1] = (x % 256).astype(np.uint8) | 1
    return out
