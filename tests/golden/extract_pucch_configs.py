"""Writes the two PUCCH fixtures from a checkout of srsRAN-5G-ER, settings and recorded results only:

  pucch_configs.json  the entries of tests/unittests/phy/upper/channel_processors/pucch_processor_format0_test_data.h and
                      pucch_processor_format1_test_data.h: the configuration and the expected HARQ-ACK (and SR) bits.  Format
                      1's entries come in pairs that share a grid ("case" numbers the pair).  The tests' vector files are not
                      used: tests/test_pucch.py builds its own grids.
  pucch_tables.json   the numbers of two tables of TS 38.211: phi(n) of the 30 low-PAPR base sequences of length 12 (Table
                      5.2.2.2-2; lib/phy/upper/sequence_generators/low_papr_sequence_generator_impl.cpp) and phi(m) of the
                      orthogonal sequences of PUCCH format 1 (Table 6.3.2.4.1-2; include/srsran/phy/upper/
                      pucch_orthogonal_sequence.h), row [N - 1][i] holding N numbers.

    python tests/golden/extract_pucch_configs.py [REFERENCE_ROOT] [OUTPUT_DIR]
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.join("tests", "unittests", "phy", "upper", "channel_processors")
LOW_PAPR = os.path.join("lib", "phy", "upper", "sequence_generators", "low_papr_sequence_generator_impl.cpp")
OCC = os.path.join("include", "srsran", "phy", "upper", "pucch_orthogonal_sequence.h")

LIST = r"\{([0-9, ]*)\}"
F0 = re.compile(r"\{\{\{std::nullopt, \{(\d+), (\d+)\}, cyclic_prefix::NORMAL, (\d+), (\d+), (\d+), " + LIST +
                r", (\d+), (\d+), (\d+), (\d+), (\d+), (true|false), " + LIST + r"\}, " + LIST + ", " + LIST + r"\}, \{\"")
F1 = re.compile(r"\{\{std::nullopt, \{(\d+), (\d+)\}, (\d+), (\d+), cyclic_prefix::NORMAL, (\d+), " + LIST +
                r", (\d+), (\d+), " + LIST + r", (\d+), (\d+), (\d+), (\d+)\}, " + LIST + r"\}")


def ints(text):
    return [int(x) for x in re.findall(r"\d+", text)]


def configs(reference_root):
    out = []
    text = open(os.path.join(reference_root, TESTS, "pucch_processor_format0_test_data.h")).read()
    for m in F0.finditer(text):
        g = m.groups()
        hop = ints(g[5])
        sr = ints(g[14])
        out.append({"format": 0, "numerology": int(g[0]), "slot_count": int(g[1]), "bwp_size_rb": int(g[2]), "bwp_start_rb": int(g[3]),
                    "starting_prb": int(g[4]), "second_hop_prb": hop[0] if hop else None, "start_symbol_index": int(g[6]),
                    "nof_symbols": int(g[7]), "initial_cyclic_shift": int(g[8]), "n_id": int(g[9]), "nof_harq_ack": int(g[10]),
                    "sr_opportunity": g[11] == "true", "ports": ints(g[12]), "ack_bits": ints(g[13]), "sr": sr[0] if sr else None})
    text = open(os.path.join(reference_root, TESTS, "pucch_processor_format1_test_data.h")).read()
    for case, line in enumerate(l for l in text.split("\n") if "std::nullopt" in l):
        for m in F1.finditer(line):
            g = m.groups()
            hop = ints(g[5])
            out.append({"format": 1, "case": case, "numerology": int(g[0]), "slot_count": int(g[1]), "bwp_size_rb": int(g[2]),
                        "bwp_start_rb": int(g[3]), "starting_prb": int(g[4]), "second_hop_prb": hop[0] if hop else None,
                        "n_id": int(g[6]), "nof_harq_ack": int(g[7]), "ports": ints(g[8]), "initial_cyclic_shift": int(g[9]),
                        "nof_symbols": int(g[10]), "start_symbol_index": int(g[11]), "time_domain_occ": int(g[12]),
                        "ack_bits": ints(g[13])})
    return out


def tables(reference_root):
    text = open(os.path.join(reference_root, LOW_PAPR)).read()
    body = text[text.index("phi_M_sc_12 = {"):text.index("phi_M_sc_18 = {")]
    phi = [[int(x) for x in re.findall(r"-?\d+", row)] for row in re.findall(r"\{([-0-9, ]+)\}", body)]
    assert len(phi) == 30 and all(len(r) == 12 for r in phi)
    text = open(os.path.join(reference_root, OCC)).read()
    body = text[text.index("pucch_format1_phi = {"):text.index("w_array orthogonal_sequence;")]
    rows = [ints(row) for row in re.findall(r"\{([0-9, ]+)\}", body)]
    occ, k = [], 0
    for n in range(1, 8):
        occ.append(rows[k:k + n])
        assert all(len(r) == n for r in occ[-1]), n
        k += n
    assert k == len(rows)
    return {"phi_12": phi, "occ_phi": occ}


def render(items):
    return "[\n" + ",\n".join(json.dumps(c, sort_keys=False) for c in items) + "\n]\n"


def render_tables(t):
    return "{\n" + ",\n".join('"%s": [\n%s\n]' % (k, ",\n".join(json.dumps(r) for r in v)) for k, v in t.items()) + "\n}\n"


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SRSRAN_ROOT", "srsRAN-5G-ER")
    dst = sys.argv[2] if len(sys.argv) > 2 else HERE
    c, t = configs(root), tables(root)
    open(os.path.join(dst, "pucch_configs.json"), "w").write(render(c))
    open(os.path.join(dst, "pucch_tables.json"), "w").write(render_tables(t))
    print("%d configurations, %d + %d table rows -> %s" % (len(c), len(t["phi_12"]), sum(len(r) for r in t["occ_phi"]), dst))
