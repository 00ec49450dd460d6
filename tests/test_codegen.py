"""Code-generation guards on the built library (no GPU needed): the device code objects are taken out of librrdxr.so and the
kernels this round put on a diet are checked for what the diet removed -- scalar registers spilled through vector lanes
(v_readlane / v_writelane: vector instructions that do no work), scratch in the hot kernels.  The compiler's choices here turned
out to hinge on details as remote as the layout of an argument struct, so a change that brings the spills back
should fail a test, not wait for a benchmark."""
import pytest

from codeobj import HAVE_OBJDUMP, kernels


@pytest.mark.skipif(not HAVE_OBJDUMP, reason="llvm-objdump of the ROCm toolchain not found")
def test_hot_kernels_do_not_spill_scalars_through_vector_lanes(tmp_path):
    k = kernels(tmp_path)

    def find(sub):
        hits = [(n, v) for n, v in k.items() if sub in n]
        assert hits, "kernel not found in the code objects: " + sub
        return hits

    # the headline kernel: 491 lane moves in 1 362 vector instructions before its diet, 49 in 906 after
    for n, v in find("k_render_lds<12, 2, false, false>"):
        assert v["lane"] <= 80 and v["scratch"] == 0, (n, v)
    # the L1-fed kernel of the reference's scene: 43 before the store's arguments were read again from the argument block, 13 after
    for n, v in find("k_render_fused<19, 2, false, false, false, unsigned int, 0>"):
        assert v["lane"] <= 30, (n, v)
    # the stream renderer's chain kernel: no scalar spills, no scratch
    for n, v in find("k_stream_rays<30, false, unsigned short, 2, 6>"):
        assert v["lane"] <= 10 and v["scratch"] == 0, (n, v)
