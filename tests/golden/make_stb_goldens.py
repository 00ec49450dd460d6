"""Regenerates tests/golden/stb_decode.npz: what the reference's own stb_image.h (v2.28) returns from stbi_loadf for
every file the *_vs_reference_stb tests of tests/test_host.py decode.

Needs oracle/_ref/libstb_ref.so, which `make -C oracle` builds only where the reference tree is present; the tests
themselves read the stored results and need nothing outside the repository.  Per key: the float32 array itself (or, for
envmap.png, its shape and FNV-1a 64 hash) and the channel count stbi_loadf reported.
    python tests/golden/make_stb_goldens.py
"""
import ctypes as C
import os
import pathlib
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import oracle as O                                   # noqa: E402
import test_host as T                                # noqa: E402  (the tests' own file writers)

REF_STB = os.path.join(ROOT, "oracle", "_ref", "libstb_ref.so")


def ref_loadf(path, req):
    L = C.CDLL(REF_STB)
    L.stbi_loadf.restype = C.POINTER(C.c_float)
    L.stbi_loadf.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    L.stbi_image_free.argtypes = [C.c_void_p]
    x, y, n = C.c_int(), C.c_int(), C.c_int()
    p = L.stbi_loadf(str(path).encode(), C.byref(x), C.byref(y), C.byref(n), req)
    if not p:
        raise RuntimeError("stbi_loadf refused %s" % path)
    oc = req if req else n.value
    a = np.ctypeslib.as_array(p, shape=(y.value, x.value, oc)).copy()
    L.stbi_image_free(p)
    return a, n.value


def main():
    if not os.path.exists(REF_STB):
        raise SystemExit("%s is missing: build it with `make -C oracle` where the reference tree is present" % REF_STB)
    out = {}

    def store(key, path, req):
        a, n = ref_loadf(path, req)
        out[key + "/n"] = np.int32(n)
        if os.path.basename(str(path)) == "envmap.png":
            out[key + "/shape"] = np.array(a.shape, np.int64)
            out[key + "/fnv1a64"] = np.uint64(O.fnv1a64(a))
        else:
            out[key] = a

    with tempfile.TemporaryDirectory() as d:
        for req in (0, 1, 2, 3, 4):
            t = pathlib.Path(d, "png%d" % req)
            t.mkdir()
            for name, p in T.png_decode_cases(t, req):
                store("png/%d/%s" % (req, name), p, req)
        t = pathlib.Path(d, "hdr")
        t.mkdir()
        hdr = T.hdr_decode_cases(t)
        for req in (0, 1, 3, 4):
            for name, p in hdr:
                store("hdr/%d/%s" % (req, name), p, req)
        t = pathlib.Path(d, "adam7")
        t.mkdir()
        adam7 = T.adam7_decode_cases(t)
        for req in (0, 3):
            for name, p in adam7:
                store("adam7/%d/%s" % (req, name), p, req)
    np.savez_compressed(os.path.join(HERE, "stb_decode.npz"), **out)
    print("%d entries" % sum(1 for k in out if k.endswith("/n")))


if __name__ == "__main__":
    main()
