"""Builds csrc/libmi355nrphy.so for gfx950 with hipcc (cross-compiles without a GPU).

    python srsran-edgeric-5g_amd/build.py [--force]

The library is built in-tree so that it travels with the repository snapshot to the GPU box.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, "libmi355nrphy.so")
SOURCES = ["nrphy_host.cpp", "pdsch_plan_build.cpp", "pdsch_host.cpp", "dl_control_host.cpp", "pdsch_async.cpp", "dl_slot_async.cpp", "ul_slot_async.cpp", "prach_window_async.cpp",
           "ofdm_host.cpp", "lower_phy_host.cpp", "demod_host.cpp", "ldpc_dematcher_host.cpp", "ldpc_decoder_host.cpp", "pusch_decoder_host.cpp",
           "csi_rs_host.cpp", "pdsch_kernels.hip", "ofdm_kernels.hip", "ldpc_decoder.hip",
           "ldpc_dematcher.hip", "pusch_decoder.hip", "csi_rs_kernels.hip", "dl_control_kernels.hip", "lower_phy_kernels.hip", "demod_kernels.hip",
           "pusch_demod_host.cpp", "pusch_demod_kernels.hip", "pusch_chest_host.cpp", "pusch_chest_kernels.hip", "pusch_chest_lowpapr_kernels.hip",
           "prach_host.cpp", "prach_kernels.hip", "prach_demod_host.cpp", "prach_demod_kernels.hip", "pucch_host.cpp", "pucch_kernels.hip",
           "pucch2_host.cpp", "pucch2_kernels.hip", "srs_host.cpp", "srs_kernels.hip",
           "uci_host.cpp", "uci_kernels.hip", "ulsch_host.cpp", "ulsch_kernels.hip", "ofh_ul_host.cpp", "ofh_ul_kernels.hip",
           "ofh_dl_host.cpp", "ofh_dl_kernels.hip", "ofh_rx_host.cpp", "ofh_rx_kernels.hip",
           "transform_precoder_host.cpp", "transform_precoder_kernels.hip", "pusch_proc_host.cpp", "pusch_proc_kernels.hip",
           "pusch_csi2_host.cpp", "pusch_csi2_kernels.hip"]
HEADERS = ["nrphy_internal.h", "nrphy_host_internal.h", "pdsch_plan.h", "pdsch_staging_host.h", "slot_pool_host.h", "ul_slot_state_host.h", "prach_window_state_host.h", "ldpc_receive_host.h", "ldpc_base_graph_host.h", "pusch_alloc_host.h", "ulsch_placement_host.h", "ulsch_info_host.h", "pusch_csi2_host.h", "pusch_proc_plan_host.h", "pusch_select_host.h", "nrphy_trace.h", "bits_device.h", "crc24b_fold.h", "ofh_compress_device.h", "ofh_ul_chunk_device.h", "chest_device.h", "chest_host.h", "pusch_chest_kernel_device.h", "low_papr_device.h", "low_papr_host.h", "demod_device.h", "equalize_device.h", "exact_device.h", "ldpc_device.h", "codeblock_build_device.h", "rate_match_device.h", "re_map_device.h", "pdsch_dmrs_device.h", "fft_device.h", "dft_mixed_device.h","nr_ldpc_bg.inc", "nr_polar_tables.inc", "prach_tables.inc", "prach_demod_tables.inc", "pucch_tables.inc", "srs_tables.inc", "pusch_lowpapr_tables.inc", "uci_tables.inc",
           os.path.join(ROOT, "include", "mi355_nrphy.h")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MAX_COMPILERS = 16  # in flight at once
# Contraction is off everywhere: the kernels say where they want a fused multiply-add (explicit __fmaf_rn / v_pk_fma_f32).  Until
# late round 4 the FFT file was built with -ffp-contract=fast; under that flag the backend fuses across `#pragma clang fp
# contract(off)`, which cost the wire-format sink its exact rounding (profiles/r04_fuzz_sweep_summary.txt), and the transforms of
# the sizes that matter (powers of two) come out instruction for instruction the same without it -- the 3 * 2^k sizes lose 4-12 of
# ~630-880 vector instructions per symbol.
CONTRACT = {}
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + [h if os.path.isabs(h) else os.path.join(CSRC, h) for h in HEADERS]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    """Compiles every HIP source for gfx950 and links the shared library; returns its path."""
    if not force and not _stale():
        return LIB
    objs = []
    cmds = []
    for src in SOURCES:
        obj = os.path.join(CSRC, os.path.splitext(src)[0] + ".o")
        cmds.append([HIPCC] + FLAGS + [CONTRACT.get(src, "-ffp-contract=off"), "-x", "hip", "-c", os.path.join(CSRC, src),
                     "-o", obj])
        objs.append(obj)
    procs = []
    try:
        while cmds or procs:
            while cmds and len(procs) < MAX_COMPILERS:
                cmd = cmds.pop(0)
                if verbose:
                    print(" ".join(cmd))
                procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
            cmd, p = procs.pop(0)
            out, _ = p.communicate(timeout=1800)
            if p.returncode != 0:
                raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), out.decode(errors="replace")))
            if verbose and out:
                print(out.decode(errors="replace"))
    finally:
        for _, p in procs:
            p.kill()
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
    subprocess.run(cmd, check=True, timeout=600)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
