"""Writes tests/golden/pf2_configs.json from a checkout of srsRAN-5G-ER: the configurations (settings only, no vectors) of the
reference's PUCCH format 2 unit tests.

  "processor"    the entries of tests/unittests/phy/upper/channel_processors/pucch_processor_format2_test_data.h
  "demodulator"  the entries of pucch_demodulator_format2_test_data.h (grid size, noise variance, ports, first PRB, sizes, rnti, n_id)
  "dmrs"         the format 2 rows of tests/unittests/phy/upper/signal_processors/dmrs_pucch_processor_test_data.h
  "validator"    pucch_processor_validator_format2_test.cpp: its base configuration and, per refused case, the fields the case sets
                 (their values worked out from the case's expressions) and the start of the message it expects

    python tests/golden/extract_pf2_configs.py [REFERENCE_ROOT] [OUTPUT_DIR]
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CP = os.path.join("tests", "unittests", "phy", "upper", "channel_processors")
SP = os.path.join("tests", "unittests", "phy", "upper", "signal_processors")

LIST = r"\{([0-9, ]*)\}"
PROC = re.compile(r"\{\{(\d+), (\d+), \{std::nullopt, \{(\d+), (\d+)\}, cyclic_prefix::NORMAL, " + LIST + r", (\d+), (\d+), (\d+), " + LIST +
                  r", (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\}\}")
DEMOD = re.compile(r"\{\{(\d+), (\d+), ([0-9.e+-]+), \{" + LIST + r", (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\}\}")
DMRS = re.compile(r"\{\{pucch_format::FORMAT_2, \{(\d+), (\d+)\}, cyclic_prefix::NORMAL, pucch_group_hopping::NEITHER, (\d+), (\d+), (\d+), "
                  r"(true|false), (\d+), (\d+), (\d+), (\d+), (true|false), (\d+), (\d+), " + LIST + r"\}")
BASE_FIELDS = ("numerology", "slot_index", "rx_ports", "bwp_size_rb", "bwp_start_rb", "starting_prb", "second_hop_prb", "nof_prb",
               "start_symbol_index", "nof_symbols", "rnti", "n_id", "n_id_0", "nof_harq_ack", "nof_sr", "nof_csi_part1", "nof_csi_part2")
# What the validator test's expressions refer to: constants of the reference and the dimensions the test builds its processor with.
CONSTANTS = {"MAX_RB": 275, "pucch_constants::FORMAT2_MIN_UCI_NBITS": 3, "PUCCH_F2_IMPL_MAX_NBITS": 1706,
             "uci_constants::MAX_NOF_HARQ_BITS": 1706, "max_dimensions.nof_symbols": 13, "max_dimensions.nof_rx_ports": 1,
             "get_nsymb_per_slot(entry.config.cp)": 14, "cyclic_prefix::NORMAL": 0}
RENAME = {"ports": "rx_ports"}


def ints(text):
    return [int(x) for x in re.findall(r"\d+", text)]


def processor(root):
    text = open(os.path.join(root, CP, "pucch_processor_format2_test_data.h")).read()
    out = []
    for m in PROC.finditer(text):
        g = m.groups()
        assert ints(g[8]) == [], "a second hop"
        out.append({"grid_nof_prb": int(g[0]), "grid_nof_symbols": int(g[1]), "numerology": int(g[2]), "slot_index": int(g[3]),
                    "rx_ports": ints(g[4]), "bwp_size_rb": int(g[5]), "bwp_start_rb": int(g[6]), "starting_prb": int(g[7]),
                    "nof_prb": int(g[9]), "start_symbol_index": int(g[10]), "nof_symbols": int(g[11]), "rnti": int(g[12]),
                    "n_id": int(g[13]), "n_id_0": int(g[14]), "nof_harq_ack": int(g[15]), "nof_sr": int(g[16]),
                    "nof_csi_part1": int(g[17]), "nof_csi_part2": int(g[18])})
    return out


def demodulator(root):
    text = open(os.path.join(root, CP, "pucch_demodulator_format2_test_data.h")).read()
    return [{"grid_nof_prb": int(g[0]), "grid_nof_symbols": int(g[1]), "noise_var": float(g[2]), "rx_ports": ints(g[3]),
             "first_prb": int(g[4]), "nof_prb": int(g[5]), "start_symbol_index": int(g[6]), "nof_symbols": int(g[7]), "rnti": int(g[8]),
             "n_id": int(g[9])} for g in (m.groups() for m in DEMOD.finditer(text))]


def dmrs(root):
    text = open(os.path.join(root, SP, "dmrs_pucch_processor_test_data.h")).read()
    return [{"numerology": int(g[0]), "slot_index": int(g[1]), "start_symbol_index": int(g[2]), "nof_symbols": int(g[3]),
             "starting_prb": int(g[4]), "intra_slot_hopping": g[5] == "true", "second_hop_prb": int(g[6]), "nof_prb": int(g[7]),
             "n_id": int(g[11]), "n_id_0": int(g[12]), "rx_ports": ints(g[13])} for g in (m.groups() for m in DMRS.finditer(text))]


def evaluate(expr, cfg):
    for k, v in CONSTANTS.items():
        expr = expr.replace(k, str(v))
    expr = re.sub(r"entry\.config\.(\w+)", lambda m: repr(cfg[RENAME.get(m.group(1), m.group(1))]), expr)
    if re.fullmatch(r"\{[0-9, ]*\}", expr):
        return ints(expr)
    assert re.fullmatch(r"[0-9+\-* ()]+", expr), expr
    return int(eval(expr))


def validator(root):
    text = open(os.path.join(root, CP, "pucch_processor_validator_format2_test.cpp")).read()
    body = text[text.index("base_format_2_config = {"):]
    body = re.sub(r"//[^\n]*", "", body[:body.index("};")])
    body = body.replace("pucch_constants::FORMAT2_MIN_UCI_NBITS", "3").replace("std::nullopt,", "").replace("cyclic_prefix::NORMAL,", "")
    tokens = re.findall(r"\{[0-9, ]*\}|\d+", body[body.index("{") + 1:])
    slot = ints(tokens[0])
    values = [slot[0], slot[1]] + [ints(t) if t.startswith("{") else int(t) for t in tokens[1:]]
    base = dict(zip(BASE_FIELDS, values))
    assert len(values) == len(BASE_FIELDS) and base["second_hop_prb"] == []
    base["second_hop_prb"] = None
    cases = []
    for block in text[text.index("pucch_processor_validator_test_data = {"):text.index("class PucchProcessorFormat2Fixture")].split("[] {")[1:]:
        cfg, sets = dict(base), {}
        for name, expr in re.findall(r"entry\.config\.(\w+)\s*=\s*([^;]+);", block):
            if name == "cp":
                continue
            name = RENAME.get(name, name)
            cfg[name] = sets[name] = evaluate(" ".join(expr.split()), cfg)
        message = re.search(r'R"\(([^"]*?)[\\{(\[]', block).group(1).strip()
        cases.append({"sets": sets, "message": message})
    return {"base": base, "cases": cases}


def render(doc):
    parts = []
    for key in ("processor", "demodulator", "dmrs"):
        parts.append('"%s": [\n%s\n]' % (key, ",\n".join(json.dumps(c) for c in doc[key])))
    v = doc["validator"]
    parts.append('"validator": {\n"base": %s,\n"cases": [\n%s\n]\n}' % (json.dumps(v["base"]), ",\n".join(json.dumps(c) for c in v["cases"])))
    return "{\n" + ",\n".join(parts) + "\n}\n"


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SRSRAN_ROOT", "srsRAN-5G-ER")
    dst = sys.argv[2] if len(sys.argv) > 2 else HERE
    doc = {"processor": processor(root), "demodulator": demodulator(root), "dmrs": dmrs(root), "validator": validator(root)}
    open(os.path.join(dst, "pf2_configs.json"), "w").write(render(doc))
    print("%d processor, %d demodulator, %d DM-RS configurations, %d validator cases -> %s" %
          (len(doc["processor"]), len(doc["demodulator"]), len(doc["dmrs"]), len(doc["validator"]["cases"]), dst))
