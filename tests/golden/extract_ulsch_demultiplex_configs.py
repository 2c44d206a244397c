"""Writes ulsch_demultiplex_configs.json from a checkout of srsRAN-5G-ER, settings only: the entries of
tests/unittests/phy/upper/channel_processors/pusch/ulsch_demultiplex_test_data.h as the fields of nrphy_ulsch_demux_cfg_t
(modulation as an NRPHY_MOD_* code, dmrs_type 0 = type 1, the DM-RS symbols as a bit mask).  The tests' vector files are not
used: the recorded inputs and answers come from record_ulsch_demultiplex_reference.cpp.

    python tests/golden/extract_ulsch_demultiplex_configs.py [REFERENCE_ROOT] [OUTPUT_DIR]
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TEST_DATA = os.path.join("tests", "unittests", "phy", "upper", "channel_processors", "pusch", "ulsch_demultiplex_test_data.h")
MODULATION = {"PI_2_BPSK": 0, "BPSK": 1, "QPSK": 2, "QAM16": 4, "QAM64": 6, "QAM256": 8}
CASE = re.compile(r"\{\{\{modulation_scheme::(\w+), (\d+), (\d+), (\d+), (\d+), (\d+), dmrs_type::TYPE(\d), \{([01, ]+)\}, (\d+), (\d+), (\d+), "
                  r"(\d+), (\d+)\}, (\d+), (\d+)\}, \{\"")


def configs(reference_root):
    text = open(os.path.join(reference_root, TEST_DATA)).read()
    out = []
    for m in CASE.findall(text):
        mask = sum(int(b) << l for l, b in enumerate(m[7].split(",")))
        out.append({"modulation": MODULATION[m[0]], "nof_layers": int(m[1]), "nof_prb": int(m[2]), "start_symbol_index": int(m[3]),
                    "nof_symbols": int(m[4]), "dmrs_type": int(m[6]) - 1, "dmrs_symbol_mask": mask,
                    "nof_cdm_groups_without_data": int(m[8]), "nof_harq_ack_rvd": int(m[5]), "nof_harq_ack_bits": int(m[9]),
                    "nof_enc_harq_ack_bits": int(m[10]), "nof_csi_part1_bits": int(m[11]), "nof_enc_csi_part1_bits": int(m[12]),
                    "nof_csi_part2_bits": int(m[13]), "nof_enc_csi_part2_bits": int(m[14])})
    return out


def render(items):
    return "[\n" + ",\n".join(json.dumps(c, sort_keys=False) for c in items) + "\n]\n"


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SRSRAN_ROOT", "srsRAN-5G-ER")
    dst = sys.argv[2] if len(sys.argv) > 2 else HERE
    c = configs(root)
    open(os.path.join(dst, "ulsch_demultiplex_configs.json"), "w").write(render(c))
    print("%d configurations -> %s" % (len(c), dst))
