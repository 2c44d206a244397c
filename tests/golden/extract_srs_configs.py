"""Writes the two SRS fixtures from a checkout of srsRAN-5G-ER, settings, table numbers and recorded results only:

  srs_configs.json  "estimator": the entries of tests/unittests/phy/upper/signal_processors/srs/srs_estimator_test_data.h -- the
                    configuration, and the channel matrix (row-major [rx][tx] pairs of re, im) and time alignment the entry expects.
                    The tests' vector files are not used: tests/golden/record_srs_reference.cpp builds its own grids.
                    "validator": srs_estimator_validator_test.cpp -- its base configuration and, per refused case, the fields
                    the case sets.
  srs_tables.json   the numbers of two tables of TS 38.211: "bandwidth", Table 6.4.1.4.3-1 as [C_SRS][B_SRS] pairs (m_SRS, N)
                    (lib/ran/srs/srs_bandwidth_configuration.cpp), and "phi_24", phi(n) of the 30 low-PAPR base sequences of length
                    24 (Table 5.2.2.2-4; lib/phy/upper/sequence_generators/low_papr_sequence_generator_impl.cpp).

    python tests/golden/extract_srs_configs.py [REFERENCE_ROOT] [OUTPUT_DIR]
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.join("tests", "unittests", "phy", "upper", "signal_processors", "srs")
LOW_PAPR = os.path.join("lib", "phy", "upper", "sequence_generators", "low_papr_sequence_generator_impl.cpp")
BANDWIDTH = os.path.join("lib", "ran", "srs", "srs_bandwidth_configuration.cpp")

FIELDS = ("nof_antenna_ports", "nof_symbols", "start_symbol", "configuration_index", "sequence_id", "bandwidth_index", "comb_size",
          "comb_offset", "cyclic_shift", "freq_position", "freq_shift", "freq_hopping")
E = r"srs_resource_configuration::\w+\((\d+)\)"
ENTRY = re.compile(r"\{\{\{\{(\d+), (\d+), (\d+), (\d+)\}, \{" + E + ", " + E + r", (\d+), (\d+), (\d+), (\d+), " + E +
                   r", (\d+), (\d+), (\d+), (\d+), (\d+), srs_resource_configuration::group_or_sequence_hopping_enum::(\w+), \{\}\}, "
                   r"\{([0-9, ]*)\}\}, \{\{\{\{([^}]*)\}\}, (\d+), (\d+)\}, (\d+), \{([0-9.e+-]+)\}\}\}")
HOPPING = {"neither": 0, "group_hopping": 1, "sequence_hopping": 2}


def ints(text):
    return [int(x) for x in re.findall(r"-?\d+", text)]


def estimator(root):
    text = open(os.path.join(root, TESTS, "srs_estimator_test_data.h")).read()
    out = []
    for m in ENTRY.finditer(text):
        g = m.groups()
        cfg = {"numerology": int(g[0])}
        cfg.update(zip(FIELDS, (int(v) for v in g[4:16])))
        cfg["hopping"] = HOPPING[g[16]]
        cfg["rx_ports"] = ints(g[17])
        h = [float(v) for v in re.findall(r"-?\d+\.\d+", g[18])]
        assert len(h) == 2 * int(g[19]) * int(g[20]) and int(g[19]) == len(cfg["rx_ports"]) and int(g[20]) == cfg["nof_antenna_ports"]
        cfg["expected_channel"] = h
        cfg["expected_time_alignment_s"] = float(g[22])
        out.append(cfg)
    return out


def validator(root):
    text = open(os.path.join(root, TESTS, "srs_estimator_validator_test.cpp")).read()
    body = text[text.index("base_config = {"):]
    body = body[:body.index("};")]
    hop = HOPPING[re.search(r"group_or_sequence_hopping_enum::(\w+)", body).group(1)]
    numbers = ints(re.sub(r"group_or_sequence_hopping_enum::\w+", "", body))
    base = {"numerology": numbers[0]}
    base.update(zip(FIELDS, numbers[4:16]))
    base["hopping"] = hop
    base["rx_ports"] = numbers[16:]
    cases = []
    for block in text[text.index("validator_test_data = {"):text.index("class srsEstimatorValidatorFixture")].split("[] {")[1:]:
        sets = {}
        for name, expr in re.findall(r"config\.resource\.(\w+)\s*=\s*([^;]+);", block):
            expr = expr.strip()
            if name == "comb_size":
                sets[name] = {"two": 2, "four": 4}[expr.rsplit("::", 1)[1]]
            elif name == "hopping":
                sets[name] = HOPPING[expr.rsplit("::", 1)[1]]
            else:
                sets[name] = int(expr)
        if "config.ports.clear()" in block:
            sets["rx_ports"] = []
        cases.append({"sets": sets, "message": re.search(r'R"\(([^"]*)\)"', block).group(1).replace("\\", "")})
    return {"base": base, "cases": cases}


def tables(root):
    text = open(os.path.join(root, BANDWIDTH)).read()
    columns = []
    for b in range(4):
        body = text[text.index("table%d = {" % b):]
        pairs = re.findall(r"\{(\d+), (\d+)\}", body[:body.index("};")])
        assert len(pairs) == 64
        columns.append([[int(m), int(n)] for m, n in pairs])
    bandwidth = [[columns[b][c] for b in range(4)] for c in range(64)]
    text = open(os.path.join(root, LOW_PAPR)).read()
    body = text[text.index("phi_M_sc_24 = {"):]
    phi = ints(body[body.index("{"):body.index("};")])
    assert len(phi) == 30 * 24 and all(v in (-3, -1, 1, 3) for v in phi)
    return {"bandwidth": bandwidth, "phi_24": [phi[24 * u:24 * u + 24] for u in range(30)]}


def rows(items):
    return "[\n" + ",\n".join(json.dumps(c) for c in items) + "\n]"


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SRSRAN_ROOT", "srsRAN-5G-ER")
    dst = sys.argv[2] if len(sys.argv) > 2 else HERE
    est, val, tab = estimator(root), validator(root), tables(root)
    open(os.path.join(dst, "srs_configs.json"), "w").write(
        '{\n"estimator": %s,\n"validator": {\n"base": %s,\n"cases": %s\n}\n}\n' % (rows(est), json.dumps(val["base"]), rows(val["cases"])))
    open(os.path.join(dst, "srs_tables.json"), "w").write('{\n"bandwidth": %s,\n"phi_24": %s\n}\n' % (rows(tab["bandwidth"]), rows(tab["phi_24"])))
    print("%d estimator configurations, %d validator cases, %d bandwidth rows -> %s" % (len(est), len(val["cases"]), len(tab["bandwidth"]), dst))
