"""UL-SCH information (nrphy_ul_sch_info): the UL-SCH / UCI rate-matching sizes of TS 38.212 Section 6.3.2.4.

No GPU: the POD mirrors, every row of the reference unit test's table (tests/golden/ulsch_info_configs.json: a configuration and
the ulsch_information expected for it), the extractor that wrote the fixture, and the configurations where the reference's unsigned
arithmetic would wrap, which are refused.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import pytest

import backends

abi = backends.abi
lib = backends.pkg.lib

GOLDEN = os.path.join(backends.ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "ulsch_info_configs.json")
REFERENCE = os.environ.get("SRSRAN_ROOT", "/root/reference/srsRAN-5G-ER")
CFG_FIELDS = [f[0] for f in abi.UlschInfoCfg._fields_]
INFO_FIELDS = [f[0] for f in abi.UlschInfo._fields_]


def rows():
    """The fixture's rows as {"config": {...}, "info": {...}}: "common" holds the fields every row agrees on, "rows" the others."""
    doc, out = json.load(open(FIXTURE)), []
    for values in doc["rows"]:
        row = {"config": {}, "info": {}}
        for k, v in dict(doc["common"], **dict(zip(doc["fields"], values))).items():
            row[k.split(".")[0]][k.split(".")[1]] = v
        out.append(row)
    return out


def as_dict(info):
    return {f: int(getattr(info, f)) for f in INFO_FIELDS}


def test_ulsch_info_pods_match_header():
    exprs = ["sizeof(nrphy_ulsch_info_cfg_t)", "sizeof(nrphy_ulsch_info_t)"]
    exprs += ["offsetof(nrphy_ulsch_info_cfg_t, %s)" % f for f in CFG_FIELDS]
    exprs += ["offsetof(nrphy_ulsch_info_t, %s)" % f for f in INFO_FIELDS]
    src = r'''#include "mi355_nrphy.h"
#include <stdio.h>
#include <stddef.h>
int main(void){size_t v[] = {%s}; for (size_t i = 0; i != sizeof v / sizeof *v; ++i) printf("%%zu ", v[i]); return 0;}''' % ", ".join(exprs)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(backends.ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")],
                       check=True, timeout=120)
        out = [int(x) for x in subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, timeout=60).stdout.split()]
    P, I = abi.UlschInfoCfg, abi.UlschInfo
    assert out == [C.sizeof(P), C.sizeof(I)] + [getattr(P, f).offset for f in CFG_FIELDS] + [getattr(I, f).offset for f in INFO_FIELDS]
    assert "nrphy_ul_sch_info" in abi.ABI_SYMBOLS and hasattr(lib.load(), "nrphy_ul_sch_info")


def test_every_row_of_the_reference_table():
    table = rows()
    assert len(table) == 432
    with_sch = without_sch = 0
    for row in table:
        assert sorted(row["config"]) == sorted(CFG_FIELDS) and sorted(row["info"]) == sorted(INFO_FIELDS)
        got = lib.ulsch_info(abi.make_ulsch_info_cfg(**row["config"]))
        assert got is not None, row["config"]
        assert as_dict(got) == row["info"], row["config"]
        with_sch += row["info"]["has_sch"]
        without_sch += 1 - row["info"]["has_sch"]
    assert with_sch > 100 and without_sch > 100
    # the table is not vacuous: every part, the reserved set, both forms, more than one codeblock
    for field in ("nof_harq_ack_re", "nof_csi_part1_re", "nof_csi_part2_re", "nof_harq_ack_rvd", "nof_ul_sch_bits"):
        assert sum(1 for r in table if r["info"][field] > 0) > 20, field
    assert any(r["info"]["nof_cb"] > 1 for r in table) and {r["info"]["base_graph"] for r in table} == {0, 1, 2}


def test_dc_overlap_bits():
    row = next(r for r in rows() if r["config"]["modulation"] == 6)
    got = lib.ulsch_info(abi.make_ulsch_info_cfg(**dict(row["config"], contains_dc=1)))
    assert as_dict(got) == dict(row["info"], nof_dc_overlap_bits=row["config"]["nof_symbols"] * 6)


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not on this machine")
def test_ulsch_info_extractor_reproduces_the_committed_fixture():
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([sys.executable, os.path.join(GOLDEN, "extract_ulsch_info_configs.py"), REFERENCE, d], check=True, timeout=120)
        name = "ulsch_info_configs.json"
        assert open(os.path.join(d, name)).read() == open(os.path.join(GOLDEN, name)).read()


# One PRB, 14 symbols, DM-RS on symbol 2: 156 RE can carry UCI, 132 of them from the DM-RS symbol on, 156 RE in all (two CDM groups
# without data leave the DM-RS symbol empty).  QPSK at R = 1/2: R Qm = 1, so without UL-SCH the left-hand side is (O + L) beta.
BASE = dict(tbs_bits=0, modulation=2, target_code_rate=512.0, nof_harq_ack_bits=0, nof_csi_part1_bits=0, nof_csi_part2_bits=0,
            alpha_scaling=1.0, beta_offset_harq_ack=20.0, beta_offset_csi_part1=6.25, beta_offset_csi_part2=6.25, nof_rb=1,
            start_symbol_index=0, nof_symbols=14, dmrs_type=1, dmrs_symbol_mask=1 << 2, nof_cdm_groups_without_data=2, nof_layers=1,
            contains_dc=0)


@pytest.mark.parametrize("name,change,want", [
    # (O + L) beta = 111 x 20 RE wanted; alpha 1 caps HARQ-ACK at 132 RE, CSI part 1 takes the other 24
    ("without UL-SCH, alpha 1", dict(nof_harq_ack_bits=100, nof_csi_part1_bits=10), dict(nof_harq_ack_re=132, nof_csi_part1_re=24)),
    # alpha 2 caps HARQ-ACK at 264 RE: N_RE - Q'_ACK = 156 - 264 wraps
    ("CSI part 1 without UL-SCH: N_RE below Q'_ACK", dict(nof_harq_ack_bits=100, nof_csi_part1_bits=10, alpha_scaling=2.0), None),
    ("CSI part 2 without UL-SCH: N_RE below Q'_ACK", dict(nof_harq_ack_bits=100, nof_csi_part2_bits=10, alpha_scaling=2.0), None),
    # the same HARQ-ACK next to a transport block of 32 bits (one codeblock of 80 bits): 156 RE in all, 264 taken
    ("UL-SCH: fewer RE than the UCI took", dict(tbs_bits=32, nof_harq_ack_bits=100, alpha_scaling=2.0), None),
    ("UL-SCH, alpha 1", dict(tbs_bits=32, nof_harq_ack_bits=100), dict(nof_harq_ack_re=132, nof_ul_sch_bits=48)),
    # conversions the reference leaves undefined
    ("a negative alpha", dict(nof_harq_ack_bits=4, alpha_scaling=-1.0), None),
    ("a beta offset that is not a number", dict(nof_harq_ack_bits=4, beta_offset_harq_ack=float("nan")), None),
    ("an infinite beta offset", dict(nof_csi_part1_bits=4, tbs_bits=32, beta_offset_csi_part1=float("inf")), None),
    # the reference's assertions
    ("a code rate of 1", dict(tbs_bits=32, target_code_rate=1024.0), None), ("a code rate of 0", dict(target_code_rate=0.0), None),
    ("3 CDM groups, type 1", dict(nof_cdm_groups_without_data=3), None),
    ("3 CDM groups, type 2", dict(nof_cdm_groups_without_data=3, dmrs_type=2), dict()),
    ("no DM-RS symbol", dict(dmrs_symbol_mask=0), None),
    ("a DM-RS symbol before the allocation", dict(start_symbol_index=3, nof_symbols=11), None),
    ("a DM-RS symbol behind the allocation", dict(nof_symbols=2), None),
    ("symbols beyond the slot", dict(start_symbol_index=1), None), ("an unknown modulation", dict(modulation=3), None),
    ("no PRB", dict(nof_rb=0), None), ("276 PRB", dict(nof_rb=276), None), ("5 layers", dict(nof_layers=5), None),
    ("the base case", dict(), dict(nof_ul_sch_bits=0, nof_harq_ack_rvd=2 * 40)),
])
def test_ulsch_info_refusals(name, change, want):
    got = lib.ulsch_info(abi.make_ulsch_info_cfg(**dict(BASE, **change)))
    if want is None:
        assert got is None, name
    else:
        assert got is not None, name
        for k, v in want.items():
            assert getattr(got, k) == v, (name, k, getattr(got, k))
