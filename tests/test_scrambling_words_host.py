"""Host-side checks of the words form of the scrambling sequences (no GPU): what the shipped library contains for it."""
import os
import sys

import backends


def test_words_form_kernels_keep_eight_waves_per_simd():
    """Every codeblock_words_kernel_t<Qm, L> within the budget of eight waves per SIMD (<= 96 scalar, <= 64 vector registers) without
    spills, like the seeds form; the mixed kernel of the words form spills no more scalar registers than the seeds form's; the
    prologue, which stores the words, still fits eight waves per SIMD (<= 64 vector registers)."""
    sys.path.insert(0, os.path.join(backends.ROOT, "profiles"))
    import disasm_lib
    rows = disasm_lib.resources(os.path.join(backends.ROOT, "srsran-edgeric-5g_amd", "csrc", "libmi355nrphy.so"))
    by_name = {r[0]: r for r in rows}
    for qm in (2, 4, 6, 8):
        for layers in (1, 2, 3, 4):
            name, sgpr, vgpr, sgpr_spill, vgpr_spill, scratch, lds = by_name["void nrphy::codeblock_words_kernel_t<%d, %d>" % (qm, layers)]
            assert int(sgpr) <= 96 and int(vgpr) <= 64 and sgpr_spill == "0" and vgpr_spill == "0" and scratch == "0", name
    assert int(by_name["nrphy::codeblock_words_kernel"][3]) <= int(by_name["nrphy::codeblock_kernel"][3])
    assert int(by_name["nrphy::prologue_kernel"][2]) <= 64
