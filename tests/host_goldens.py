"""What the host-side tests share (test_oracle_goldens.py, test_host.py, test_host_sanitized.py): the goldens the survey recorded for
the reference's loader and camera, and hand-built Adam7-interlaced PNG files."""
import struct
import zlib

import numpy as np

# produced by the reference's own Mesh::load body (g++ 11.4)
LOADER_GOLD = {
    "cube.obj": (12, "62afee94b8d6cb6a", (-1, -1, -1), (1, 1, 1)),
    "sphere.obj": (768, "9b7d5bd5769fd643", (-1.732051,) * 3, (1.732051,) * 3),
    "monkey.obj": (967, "a4734543877c2dd5", (-1.367188, -0.984375, -1.504792), (1.367188, 0.984375, 0.198333)),
    "shell.obj": (1536, "7f2f52b6a1a28e63", (-1.732051,) * 3, (1.732051,) * 3),
    "ott.obj": (12877, "46b040642a0ffe6f", (-0.927691, -1.211907, -1.236633), (0.931792, 1.282290, 0.559067)),
}
# SURVEY Appendix A.1 (float64 evaluation, compare at 1e-5), angle 0.01
CAMERA_KATS = [
    (1024, 768, 512, 384, (-0.999943191, -0.000640168, -0.010639805)),
    (1024, 768, 0, 0, (-0.778907078, 0.379981610, 0.498916566)),
    (1024, 768, 1023, 767, (-0.768773635, -0.379981610, -0.514393889)),
    (1920, 1080, 960, 540, (-0.999946425, -0.000455231, -0.010341152)),
    (1920, 1080, 0, 0, (-0.778775816, 0.380059543, 0.499062092)),
    (1920, 1080, 1919, 1079, (-0.768639490, -0.380059543, -0.514536761)),
]
M_GOLD = np.array([[0.006501146, 0, 0, -0.9919504], [0, 0.487716015, 0, 0],
                   [-0.650092915, 0, 0, -0.009919835], [-2.600371662, 0, 1, 1.059519008]])


def _write_adam7_png(path, arr, depth=8, palette=None):
    """A PNG with interlace method 1 (Adam7) built by hand: arr is H x W (gray / palette indices, `depth` bits) or
    H x W x C with C = 2 (gray+alpha), 3 (RGB), 4 (RGBA) at 8 bits.  Rows use filter types 0, 1 and 2 in turn."""
    import struct, zlib
    h, w = arr.shape[:2]
    ch = 1 if arr.ndim == 2 else arr.shape[2]
    ctype = {1: 3 if palette is not None else 0, 2: 4, 3: 2, 4: 6}[ch]
    bits_pp = ch * depth
    bpp = max(1, bits_pp // 8)

    def pack_row(px):                       # px: n x ch samples -> bytes
        if depth == 8:
            return bytes(px.astype(np.uint8).reshape(-1))
        if depth == 16:
            return px.astype(">u2").reshape(-1).tobytes()
        bits = "".join(format(int(v), "0%db" % depth) for v in px.reshape(-1))
        bits += "0" * (-len(bits) % 8)
        return bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))

    raw = bytearray()
    for x0, y0, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
        sub = arr[y0::dy, x0::dx]
        if sub.shape[0] == 0 or sub.shape[1] == 0:
            continue
        prev = None
        for j in range(sub.shape[0]):
            cur = pack_row(sub[j].reshape(sub.shape[1], ch))
            ft = j % 3
            if ft == 1:
                out = bytes((cur[i] - (cur[i - bpp] if i >= bpp else 0)) & 255 for i in range(len(cur)))
            elif ft == 2:
                out = bytes((cur[i] - (prev[i] if prev is not None else 0)) & 255 for i in range(len(cur)))
            else:
                out = cur
            raw += bytes([ft]) + out
            prev = cur

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))
    png = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 1))
    if palette is not None:
        png += chunk(b"PLTE", bytes(np.asarray(palette, np.uint8).reshape(-1)))
    png += chunk(b"IDAT", zlib.compress(bytes(raw))) + chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(png)


def _adam7_cases(rng):
    pal = rng.integers(0, 256, (16, 3), dtype=np.uint8)
    return {
        "i_rgb.png": (rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), 8, None),
        "i_rgba.png": (rng.integers(0, 256, (9, 5, 4), dtype=np.uint8), 8, None),
        "i_la.png": (rng.integers(0, 256, (16, 17, 2), dtype=np.uint8), 8, None),
        "i_gray.png": (rng.integers(0, 256, (40, 31), dtype=np.uint8), 8, None),
        "i_g16.png": (rng.integers(0, 65536, (11, 9), dtype=np.uint16), 16, None),
        "i_g1.png": (rng.integers(0, 2, (13, 21), dtype=np.uint8), 1, None),
        "i_g2.png": (rng.integers(0, 4, (7, 3), dtype=np.uint8), 2, None),
        "i_pal4.png": (rng.integers(0, 16, (10, 19), dtype=np.uint8), 4, pal),
        "i_tiny.png": (rng.integers(0, 256, (1, 1, 3), dtype=np.uint8), 8, None),      # six of the seven passes are empty
        "i_thin.png": (rng.integers(0, 256, (3, 2, 3), dtype=np.uint8), 8, None),
    }
