"""Writes ulsch_info_configs.json from a checkout of srsRAN-5G-ER, data only: the rows of
tests/unittests/ran/pusch/ulsch_info_test_data.h, each a ulsch_configuration and the ulsch_information the reference's unit test
expects for it, as the fields of nrphy_ulsch_info_cfg_t ("config": modulation as an NRPHY_MOD_* code, the code rate times 1024 as
the header has it, dmrs_type 1 or 2, the DM-RS symbols as a bit mask; contains_dc is not set by any row) and of nrphy_ulsch_info_t
("info").  The rows list a segmentation for a PUSCH without UL-SCH too, which the reference's test does not compare: "info" keeps
has_sch 0 and zeros there.  nof_dc_overlap_bits is not part of a row; with contains_dc 0 it is 0.  The file holds the fields on
which every row agrees once ("common") and the others as one array per row, in the order of "fields".

    python tests/golden/extract_ulsch_info_configs.py [REFERENCE_ROOT] [OUTPUT_DIR]
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TEST_DATA = os.path.join("tests", "unittests", "ran", "pusch", "ulsch_info_test_data.h")
MODULATION = {"PI_2_BPSK": 0, "BPSK": 1, "QPSK": 2, "QAM16": 4, "QAM64": 6, "QAM256": 8}
NUM = r"([0-9.eE+-]+)"
BITS = r"units::bits\((\d+)\)"
CASE = re.compile(
    r"^\{\{" + BITS + r", \{modulation_scheme::(\w+), " + NUM + r"\}, " + BITS + ", " + BITS + ", " + BITS + ", " +
    ", ".join([NUM] * 4) + r", (\d+), (\d+), (\d+), dmrs_config_type::type(\d), \{([01, ]+)\}, (\d+), (\d+)\}, "
    r"\{\{\{" + BITS + r", ldpc_base_graph_type::BG(\d), (\d+), " + BITS + r", (\d+), " + BITS + r"\}\}, " +
    ", ".join([BITS] * 5) + r", (\d+), (\d+), (\d+)\}\},$", re.M)


def configs(reference_root):
    text = open(os.path.join(reference_root, TEST_DATA)).read()
    out = []
    for m in CASE.findall(text):
        tbs = int(m[0])
        config = {"tbs_bits": tbs, "modulation": MODULATION[m[1]], "target_code_rate": float(m[2]), "nof_harq_ack_bits": int(m[3]),
                  "nof_csi_part1_bits": int(m[4]), "nof_csi_part2_bits": int(m[5]), "alpha_scaling": float(m[6]),
                  "beta_offset_harq_ack": float(m[7]), "beta_offset_csi_part1": float(m[8]), "beta_offset_csi_part2": float(m[9]),
                  "nof_rb": int(m[10]), "start_symbol_index": int(m[11]), "nof_symbols": int(m[12]), "dmrs_type": int(m[13]),
                  "dmrs_symbol_mask": sum(int(b) << l for l, b in enumerate(m[14].split(","))),
                  "nof_cdm_groups_without_data": int(m[15]), "nof_layers": int(m[16]), "contains_dc": 0}
        sch = [int(v) for v in m[17:23]] if tbs > 0 else [0] * 6
        info = {"has_sch": int(tbs > 0), "tb_crc_bits": sch[0], "base_graph": sch[1], "nof_cb": sch[2], "nof_filler_bits_per_cb": sch[3],
                "lifting_size": sch[4], "nof_bits_per_cb": sch[5], "nof_ul_sch_bits": int(m[23]), "nof_harq_ack_bits": int(m[24]),
                "nof_harq_ack_rvd": int(m[25]), "nof_csi_part1_bits": int(m[26]), "nof_csi_part2_bits": int(m[27]),
                "nof_harq_ack_re": int(m[28]), "nof_csi_part1_re": int(m[29]), "nof_csi_part2_re": int(m[30]), "nof_dc_overlap_bits": 0}
        out.append({"config": config, "info": info})
    return out


def render(items):
    """Compact form: the fields every row agrees on once ("common"), the others as one array per row in the order of "fields"
    (names are "config.<field>" and "info.<field>")."""
    flat = [{"%s.%s" % (part, k): v for part in ("config", "info") for k, v in row[part].items()} for row in items]
    common = {k: v for k, v in flat[0].items() if all(f[k] == v for f in flat)}
    fields = [k for k in flat[0] if k not in common]
    cells = [json.dumps([f[k] for k in fields], separators=(",", ":")) for f in flat]
    rows = ",\n".join(", ".join(cells[i:i + 4]) for i in range(0, len(cells), 4))  # four rows to a line
    return '{"common": %s,\n"fields": %s,\n"rows": [\n%s\n]}\n' % (json.dumps(common), json.dumps(fields), rows)


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SRSRAN_ROOT", "srsRAN-5G-ER")
    dst = sys.argv[2] if len(sys.argv) > 2 else HERE
    c = configs(root)
    open(os.path.join(dst, "ulsch_info_configs.json"), "w").write(render(c))
    print("%d configurations -> %s" % (len(c), dst))
