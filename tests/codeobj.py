"""The gfx950 code objects of the built library, for the code-generation tests (no GPU needed): the one walk that takes them out
of librrdxr.so and disassembles them, and the one list of the ray-tree kernels' launchable instantiations."""
import os
import re
import shutil
import subprocess

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
HAVE_OBJDUMP = os.path.exists(OBJDUMP)

# every (STACK, PEND, TLAS, E) the ladder of the ray-tree kernels (for_tree_variant, csrc/rr_choice.h) can launch:
# launch_render_fused's ladder without its 22-entry rung.  Fourteen templates are built as these 20 -- k_shade_rays,
# k_render_samples, k_adaptive_base, k_adaptive_refine, k_render_lens, k_render_spectral, k_shade_rays_mat, k_render_materials,
# k_shade_rays_nested, k_render_nested, k_render_composed, k_render_shutter, k_shade_rays_surfaces and k_render_surfaces; tree_matrix.py
# reaches each of the 20 with a scene
LAUNCHABLE = [(30, 2, True, "unsigned short"), (39, 2, True, "unsigned short"), (39, 2, False, "unsigned short"),
              (39, 8, False, "unsigned short")] + \
             [(s, 2, t, "unsigned int") for s in (19, 26, 31, 39, 64) for t in (False, True)] + \
             [(s, 8, t, "unsigned int") for s in (31, 39, 64) for t in (False, True)]


def template_args(stack, pend, tlas, e):
    """a LAUNCHABLE entry as the demangled kernel names spell it"""
    return "<%d, %d, %s, %s>" % (stack, pend, "true" if tlas else "false", e)


def kernels(tmp_path, lib=None, lines=False):
    """{demangled symbol: {"lane": v_readlane / v_writelane, "scratch": scratch_*, "valu": v_* instructions}} of every symbol in
    the gfx950 code objects of librrdxr.so (built first if it is stale); tmp_path receives the unbundled objects.
    lib: another library or object file to walk instead; lines: every entry also gets "lines", its instruction lines as
    disassembled, without address comments and without the zero padding behind the last instruction"""
    work = tmp_path / "co"
    work.mkdir()
    so = work / "librrdxr.so"
    if lib is None:
        import refraction_raytracing_dxr_amd._build as B
        lib = B.build()
    shutil.copy(lib, so)
    subprocess.run([OBJDUMP, "--offloading", str(so)], check=True, capture_output=True, cwd=work)
    out = {}
    for f in sorted(work.iterdir()):
        if "gfx950" not in f.name:
            continue
        dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "-C", str(f)], check=True, capture_output=True, text=True).stdout
        cur = None
        for line in dis.split("\n"):
            m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
            if m:
                cur = out.setdefault(m.group(1), {"lane": 0, "scratch": 0, "valu": 0})
                if lines:
                    cur.setdefault("lines", [])
                continue
            if cur is None:
                continue
            if lines:
                text = line.split("//")[0].strip()
                if text and text != "...":
                    cur["lines"].append(text)
            ins = line.strip().split(" ")[0] if line.strip() else ""
            if ins.startswith(("v_readlane", "v_writelane")):
                cur["lane"] += 1
            if ins.startswith("scratch_"):
                cur["scratch"] += 1
            if ins.startswith("v_"):
                cur["valu"] += 1
    return out
