"""Are the gfx950 kernels of two builds the same code?  The instrument of a refactor that must not change device code.

    python3 tools/codeobj_diff.py A B        (A, B: two librrdxr.so, or two object files of one source)

Every gfx950 symbol gets a line: `same` (in both, equal instruction lines), `differs` (with both line counts), `only in A`,
`only in B`.  Address comments and the padding behind a kernel's last instruction are not compared: tests/codeobj.py leaves
out the comments and the zeros, and the s_nop fill that follows the s_endpgm of the last kernel of a .text section (which
kernel that is depends on what else its source file holds) is dropped here.  Beside the instructions the figures of every
kernel's metadata note are compared: vector, accumulator and scalar registers, spill counts, private segment and LDS size; a
kernel whose figures differ counts as `differs`.  The exit status is 0 only if every symbol is `same`.  Needs no GPU.
"""
import os
import pathlib
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import codeobj  # noqa: E402

READELF = os.path.join(os.path.dirname(codeobj.OBJDUMP), "llvm-readelf")
FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
           "group_segment_fixed_size")


def notes(work):
    """{kernel symbol (mangled): {figure: value}} from the metadata notes of the code objects codeobj.kernels() left in work"""
    out = {}
    for f in sorted(work.iterdir()):
        if "gfx950" not in f.name:
            continue
        text = subprocess.run([READELF, "--notes", str(f)], check=True, capture_output=True, text=True).stdout
        for entry in re.split(r"\n\s*- \.", text)[1:]:        # one list item per kernel (and per argument: those have no .symbol)
            fields = dict(re.findall(r"^\s*\.?(\w+):\s*(\S+)\s*$", "." + entry, re.M))
            if "symbol" in fields:
                out[fields["symbol"]] = {k: fields.get(k) for k in FIGURES}
    return out


def walk(lib, tmp):
    tmp = pathlib.Path(tmp)
    syms = codeobj.kernels(tmp, lib=lib, lines=True)
    for k in syms.values():
        n = len(k["lines"])
        while n and k["lines"][n - 1] == "s_nop 0":
            n -= 1
        if n and k["lines"][n - 1] == "s_endpgm":       # (nops that end a kernel without s_endpgm in front are code)
            del k["lines"][n:]
    return syms, notes(tmp / "co")


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        (ka, na), (kb, nb) = walk(sys.argv[1], ta), walk(sys.argv[2], tb)
    tally = {"same": 0, "differs": 0, "only in A": 0, "only in B": 0}
    for sym in sorted(set(ka) | set(kb)):
        if sym not in kb or sym not in ka:
            res = "only in A" if sym in ka else "only in B"
        elif ka[sym]["lines"] != kb[sym]["lines"]:
            res = "differs (%d / %d lines)" % (len(ka[sym]["lines"]), len(kb[sym]["lines"]))
        else:
            res = "same"
        tally[res.split(" (")[0]] += 1
        print("%-9s %s" % (res, sym) if res == "same" else "%s: %s" % (res, sym))
    bad_notes = 0
    for sym in sorted(set(na) & set(nb)):               # (a kernel of one side only has its line above)
        if na[sym] != nb[sym]:
            bad_notes += 1
            print("differs (notes): %s\n    A %s\n    B %s" % (sym, na[sym], nb[sym]))
    print("%d symbols: %s; %d kernels' notes compared, %d differ" % (len(set(ka) | set(kb)), ", ".join("%d %s" % (v, k) for k, v in tally.items()),
                                                                 len(set(na) & set(nb)), bad_notes))
    return 0 if tally["same"] == len(set(ka) | set(kb)) and bad_notes == 0 and ka else 1


if __name__ == "__main__":
    sys.exit(main())
