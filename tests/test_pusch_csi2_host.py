"""Host checks of the PUSCH processor with CSI part 2 (nrphy_pusch_csi2_*; no GPU).

The POD mirrors against the header; nrphy_pusch_csi2_validate over each refusal; nrphy_pusch_csi2_size against a NumPy restatement
of uci_part2_get_size; nrphy_pusch_csi2_variants against nrphy_ul_sch_info called here per size; and the stand-alone program
tests/pusch_csi2_check.cpp, which compiles csrc/pusch_csi2_host.h alone, built plainly and under the address and
undefined-behaviour sanitizers.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import backends
import pusch_csi2_cases as K
import test_pusch_processor as T
import uci_model

abi = backends.abi
lib = backends.pkg.lib
NPORTS, NSUBC, OPTIONS = T.NPORTS, T.NSUBC, T.OPTIONS


def test_pusch_csi2_pods_match_header():
    pods = [("nrphy_pusch_csi2_entry_t", abi.PuschCsi2Entry), ("nrphy_pusch_csi2_desc_t", abi.PuschCsi2Desc),
            ("nrphy_pusch_csi2_result_t", abi.PuschCsi2Result)]
    exprs, want = [], []
    for cname, cls in pods:
        exprs.append("sizeof(%s)" % cname)
        want.append(C.sizeof(cls))
        exprs.append("_Alignof(%s)" % cname)
        want.append(C.alignment(cls))
        for f in cls._fields_:
            exprs.append("offsetof(%s, %s)" % (cname, f[0]))
            want.append(getattr(cls, f[0]).offset)
    exprs += ["NRPHY_PUSCH_CSI2_MAX_ENTRIES", "NRPHY_PUSCH_CSI2_MAX_PARAMETERS", "NRPHY_PUSCH_CSI2_MAX_ENTRY_BITS",
              "NRPHY_PUSCH_CSI2_MAX_SIZES", "NRPHY_PUSCH_CSI2_MAX_VARIANTS"]
    want += [abi.PUSCH_CSI2_MAX_ENTRIES, abi.PUSCH_CSI2_MAX_PARAMETERS, abi.PUSCH_CSI2_MAX_ENTRY_BITS, abi.PUSCH_CSI2_MAX_SIZES,
             abi.PUSCH_CSI2_MAX_VARIANTS]
    src = r'''#include "mi355_nrphy.h"
#include <stdio.h>
#include <stddef.h>
int main(void){size_t v[] = {%s}; for (size_t i = 0; i != sizeof v / sizeof *v; ++i) printf("%%zu ", v[i]); return 0;}''' % ", ".join(exprs)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(backends.ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")],
                       check=True, timeout=120)
        out = [int(x) for x in subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, timeout=60).stdout.split()]
    assert out == want
    assert C.sizeof(abi.PuschCsi2Result) == 32 and C.alignment(abi.PuschCsi2Result) == 8
    assert (abi.PUSCH_CSI2_MAX_ENTRIES, abi.PUSCH_CSI2_MAX_PARAMETERS, abi.PUSCH_CSI2_MAX_ENTRY_BITS, abi.PUSCH_CSI2_MAX_SIZES) == (2, 2, 4, 16)
    names = [s for s in abi.ABI_SYMBOLS if "_pusch_csi2_" in s]
    assert len(names) == 8 and not [s for s in names if not hasattr(lib.load(), s)]
    # the names stay clear of the families other tests count
    assert not [s for s in names if any(k in s for k in ("_pusch_proc_", "_ulsch_", "_uci_", "_ul_slot"))]


def pdu_of(name, **change):
    return abi.make_pusch_pdu(**dict(K.all_args()[name], **change))


G, H = K.DESCS["g"], K.DESCS["h"]


@pytest.mark.parametrize("name,case,pdu_change,entries,want", [
    ("(g)", "g", {}, G, True), ("(h)", "h", {}, H, True), ("(i)", "i", {}, K.DESCS["i"], True), ("(j)", "j", {}, K.DESCS["j"], True),
    ("(c) without description", "c", {}, (), True),
    ("a fixed size: one parameter of no bits", "g", {}, [([(0, 0)], [9])], True),
    ("a fixed size: no parameter", "g", {}, [([], [9])], True),
    ("a parameter that ends with the payload", "g", {}, [([(4, 2)], [0, 1, 2, 7])], True),
    # everything the existing validator refuses: one of its cases
    ("DM-RS type 2", "g", dict(dmrs_type=2), G, False),
    ("a PRB beyond the grid", "g", dict(prbs=range(20, 26)), G, False),
    # the description against the PDU
    ("entries the PDU does not announce", "g", dict(nof_csi_part2_entries=0), G, False),
    ("announced entries without description", "g", {}, (), False),
    ("3 entries", "h", dict(nof_csi_part2_entries=3), H + [([(0, 1)], [1, 2])], False),
    ("3 parameters", "h", dict(nof_csi_part2_entries=1), [([(0, 1), (1, 1), (2, 1)], [4] * 8)], False),
    ("widths summing to 5", "h", dict(nof_csi_part2_entries=1), [([(0, 3), (3, 2)], [4] * 32)], False),
    ("a width of 5", "h", dict(nof_csi_part2_entries=1), [([(0, 5)], [4] * 32)], False),
    ("map_size 3 for 2 bits", "g", {}, [([(1, 2)], [0, 1, 2])], False),
    ("map_size 8 for 2 bits", "g", {}, [([(1, 2)], [0, 1, 2, 7, 7, 7, 7, 7])], False),
    ("offset + width one beyond the payload", "g", {}, [([(5, 2)], [0, 1, 2, 7])], False),
    ("an offset that wraps", "g", {}, [([(0xFFFFFFFF, 2)], [0, 1, 2, 7])], False),
    ("a description without CSI part 1", "b", dict(nof_csi_part2_entries=1), [([(0, 0)], [9])], False),
    ("a description without codeword", "e", dict(nof_csi_part2_entries=1), [([(0, 1)], [0, 9])], False),
    ("400 bits", "i", {}, [([(0, 1)], [40, 400])], True),
    ("a size above 1706", "i", {}, [([(0, 1)], [40, 1707])], False),
    ("a sum above 1706", "h", {}, [([(0, 1), (5, 2)], [900] * 8), ([(10, 2)], [0, 0, 12, 807])], False),
    ("16 distinct sizes", "h", dict(nof_csi_part2_entries=1), [([(0, 4)], list(range(12, 28)))], True),
    ("17 distinct sizes", "h", {}, [([(0, 4)], list(range(12, 28))), ([(10, 2)], [0, 0, 0, 16])], False),
    # a variant a stage refuses: part 2 finds no RE left (alpha caps the UCI REs and part 1 takes them all)
    ("no soft bit left for part 2", "h", dict(alpha_scaling=0.02), H, False),
])
def test_pusch_csi2_validator(name, case, pdu_change, entries, want):
    pdu = pdu_of(case, **pdu_change)
    desc = abi.make_pusch_csi2_desc(entries)
    assert (lib.pusch_csi2_validate(pdu, desc, OPTIONS, NPORTS, NSUBC) == abi.OK) == want, name
    assert (lib.pusch_csi2_variants(pdu, desc, OPTIONS, NPORTS, NSUBC) is not None) == want, name


def test_the_case_without_a_soft_bit_is_what_it_claims():
    """With alpha 0.02, (h) without part 2 is accepted; HARQ-ACK and part 1 take every RE the cap allows, so G^CSI-2 is 0."""
    a = dict(K.all_args()["h"], alpha_scaling=0.02)
    assert lib.pusch_proc_validate(abi.make_pusch_pdu(**dict(a, nof_csi_part2_entries=0)), OPTIONS, NPORTS, NSUBC) == abi.OK
    info = lib.ulsch_info(abi.make_ulsch_info_cfg(**info_fields(a, 12)))
    assert info is not None and info.nof_csi_part1_bits > 0 and info.nof_csi_part2_bits == 0


def test_the_existing_processor_keeps_refusing_a_description():
    for name in "ghij":
        assert lib.pusch_proc_validate(pdu_of(name), OPTIONS, NPORTS, NSUBC) == abi.ERR_ARGUMENT
        assert lib.pusch_proc_validate(pdu_of(name, nof_csi_part2_entries=0), OPTIONS, NPORTS, NSUBC) == abi.OK


def random_description(rng, nof_bits):
    entries = []
    for _ in range(int(rng.integers(1, 3))):
        left, parameters = 4, []
        for _ in range(int(rng.integers(0, 3))):
            width = int(rng.integers(0, min(left, nof_bits) + 1))
            parameters.append((int(rng.integers(0, nof_bits - width + 1)), width))
            left -= width
        entries.append((parameters, [int(v) for v in rng.integers(0, 200, 1 << (4 - left))]))
    return entries


def test_size_against_the_restatement():
    rng = np.random.default_rng(31)
    seen_widths = set()
    for _ in range(200):
        nof_bits = int(rng.integers(1, 60))
        entries = random_description(rng, nof_bits)
        desc = abi.make_pusch_csi2_desc(entries)
        seen_widths |= {w for parameters, _ in entries for _, w in parameters}
        for _ in range(4):
            bits = rng.integers(0, 2, nof_bits, dtype=np.uint8)
            assert lib.pusch_csi2_size(desc, bits) == K.size_restated(entries, bits), (entries, bits)
    assert seen_widths == {0, 1, 2, 3, 4}
    # a missing bit reversal: width 2 with map[1] != map[2] -- the payload bit at `offset` is the most significant, as the recording
    # of the reference shows (tests/test_pusch_csi2.py)
    g = abi.make_pusch_csi2_desc(G)
    assert [lib.pusch_csi2_size(g, b) for b in ([0, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 1, 1, 0, 0, 0])] == [0, 2, 1, 7]
    # a swapped parameter order: two parameters of different widths, the first one in the high bit of the index
    two = abi.make_pusch_csi2_desc([([(0, 1), (5, 2)], [10, 11, 12, 13, 14, 15, 16, 17])])
    bits = lambda *ones: [int(i in ones) for i in range(8)]
    assert [lib.pusch_csi2_size(two, bits(*o)) for o in ((0,), (5,), (6,), (0, 5, 6))] == [14, 12, 11, 17]
    # only the structure is checked here, against the payload's length
    assert lib.pusch_csi2_size(g, [0, 1]) is None and lib.pusch_csi2_size(abi.make_pusch_csi2_desc(()), [0, 1]) is None
    for name in "ghij":
        rng = np.random.default_rng(5)
        for size in K.SELECTABLE[name]:
            assert lib.pusch_csi2_size(K.desc_of(name), K.part1_for(name, size, rng)) == size


def info_fields(a, size):
    """The keyword arguments of abi.make_ulsch_info_cfg for a PDU (keyword arguments of make_pusch_pdu) with part 2 of `size` bits."""
    prbs, dc = list(a["prbs"]), a.get("dc_position")
    return dict(tbs_bits=8 * a["tb_size_bytes"], modulation=a["modulation"], target_code_rate=a["target_code_rate"],
                nof_harq_ack_bits=a.get("nof_harq_ack", 0), nof_csi_part1_bits=a.get("nof_csi_part1", 0), nof_csi_part2_bits=size,
                alpha_scaling=a["alpha_scaling"], beta_offset_harq_ack=a["beta_offset_harq_ack"],
                beta_offset_csi_part1=a["beta_offset_csi_part1"], beta_offset_csi_part2=a["beta_offset_csi_part2"], nof_rb=len(prbs),
                start_symbol_index=0, nof_symbols=14, dmrs_type=1, dmrs_symbol_mask=sum(1 << l for l in a["dmrs_symbols"]),
                nof_cdm_groups_without_data=2, nof_layers=a["nof_layers"], contains_dc=int(dc is not None and dc // 12 in prbs))


def test_variants_against_ul_sch_info_per_size():
    for name in "ghij":
        a = K.all_args()[name]
        sizes, infos = lib.pusch_csi2_variants(pdu_of(name), K.desc_of(name), OPTIONS, NPORTS, NSUBC)
        assert sizes == K.SIZES[name], name
        for size, info in zip(sizes, infos):
            want = lib.ulsch_info(abi.make_ulsch_info_cfg(**info_fields(a, size)))
            assert bytes(info) == bytes(want), (name, size)
            assert (info.nof_csi_part2_bits > 0) == (size > 0)
        assert [i.nof_ul_sch_bits for i in infos] == sorted((i.nof_ul_sch_bits for i in infos), reverse=True)
        assert len({i.nof_ul_sch_bits for i in infos}) == len(infos)  # every variant another rate-matched length
    # a PDU without description: one row, the information nrphy_pusch_proc_derive gives
    sizes, infos = lib.pusch_csi2_variants(pdu_of("c"), K.desc_of("c"), OPTIONS, NPORTS, NSUBC)
    assert sizes == [0] and bytes(infos[0]) == bytes(lib.pusch_proc_derive(pdu_of("c"), OPTIONS, NPORTS, NSUBC).info)
    for name in "ghij":
        plain = pdu_of(name, nof_csi_part2_entries=0)
        assert lib.pusch_csi2_harq_bytes(pdu_of(name), K.desc_of(name), OPTIONS) == lib.pusch_proc_harq_bytes(plain, OPTIONS)


def test_the_cases_are_what_they_claim_to_be():
    """Where the reference's streaming demultiplexer and the up-front placement agree ((g), (h), (i): what a recording of the
    reference may pin) and where they do not ((j)); the code families; the codeblocks of (i)."""
    for name in "ghij":
        base = lib.pusch_proc_derive(pdu_of(name, nof_csi_part2_entries=0), OPTIONS, NPORTS, NSUBC)
        sizes, infos = lib.pusch_csi2_variants(pdu_of(name), K.desc_of(name), OPTIONS, NPORTS, NSUBC)
        differs = [K.part2_starts_before_part1_ends(K.demux_with_part2(base.demux, s, i)) for s, i in zip(sizes[1:], infos[1:])]
        assert differs == [name == "j"] * len(differs), (name, differs)
        for s, i in zip(sizes[1:], infos[1:]):
            assert uci_model.ulsch_sizes(K.demux_with_part2(base.demux, s, i))[0] == i.nof_ul_sch_bits, (name, s)
    assert T.nof_codeblocks(pdu_of("i")) > 1 and T.nof_codeblocks(pdu_of("g")) == 1
    i_base = lib.pusch_proc_derive(pdu_of("i", nof_csi_part2_entries=0), OPTIONS, NPORTS, NSUBC)
    assert i_base.info.nof_harq_ack_rvd == i_base.info.nof_harq_ack_bits > 0  # two bits: the reserved set, all of it punctured


# =======================================================================================================================
# The stand-alone program
# =======================================================================================================================
SRC = os.path.join(backends.ROOT, "tests", "pusch_csi2_check.cpp")
INC = [os.path.join(backends.ROOT, "srsran-edgeric-5g_amd", "csrc"), os.path.join(backends.ROOT, "include")]


def build_and_run(flags):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "pusch_csi2_check")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", INC[0], "-I", INC[1]] + flags + [SRC, "-o", exe], check=True,
                       timeout=300)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.startswith("ok: "), r.stdout
        return r.stdout


def test_check_program():
    out = build_and_run(["-O2"])
    assert int(out.split()[1]) > 100000, out


def test_check_program_under_address_and_undefined_sanitizers():
    sanitize = "-fsanitize=address,undefined"
    with tempfile.TemporaryDirectory() as d:
        probe = subprocess.run(["g++", sanitize, "-x", "c++", "-", "-o", os.path.join(d, "probe")], input="int main(){return 0;}",
                               capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("this g++ has no runtime for " + sanitize)
    build_and_run(["-O1", "-g", sanitize, "-fno-sanitize-recover=all"])


def test_the_measurement_script_leaves_timing_and_limits_to_the_harness(monkeypatch):
    """profiles/pusch_csi2_measure.py under the rules tests/test_bench_harness.py holds the *_bench.py scripts to (that test counts
    those scripts, so this one has another name): --help without a device or a library, no timing and no guard of its own."""
    import contextlib
    import io
    import re
    import runpy
    import sys
    script = os.path.join(backends.ROOT, "profiles", "pusch_csi2_measure.py")
    text = open(script).read()
    assert "elapsed_time(" not in text and not re.search(r"""["']timeout["']""", text) and "subprocess" not in text
    assert "bench_harness" in text and "harness.run_steps(" in text and "harness.time_rounds(" in text
    monkeypatch.setattr(sys, "argv", [script, "--help"])
    monkeypatch.setattr(sys, "path", [os.path.join(backends.ROOT, "profiles")] + list(sys.path))
    monkeypatch.setenv("NRPHY_LIB_SO", "/nonexistent/libmi355nrphy.so")
    out = io.StringIO()
    with contextlib.redirect_stdout(out), pytest.raises(SystemExit) as stop:
        runpy.run_path(script, run_name="__main__")
    assert stop.value.code == 0 and "--help" in out.getvalue()
