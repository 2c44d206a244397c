"""Writes tests/golden/pusch_demodulator_configs.json: the 50 configurations of the reference's PUSCH demodulator unit test
(tests/unittests/phy/upper/channel_processors/pusch/pusch_demodulator_test_data.h of srsRAN-5G-ER), settings only.  The test's
vector files are not used: tests/test_pusch_demodulator.py runs these configurations on seeded synthetic grids and estimates.

    python tests/golden/extract_pusch_demod_configs.py [REFERENCE_ROOT] [OUTPUT]
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join("tests", "unittests", "phy", "upper", "channel_processors", "pusch", "pusch_demodulator_test_data.h")
OUTPUT = os.path.join(HERE, "pusch_demodulator_configs.json")

# {{noise_var, sinr_dB, {rnti, {{rb_mask}}, modulation_scheme::M, start, nof_symbols, {dmrs_symb_pos}, dmrs_type::TYPEn, cdm,
#   n_id, nof_tx_layers, enable_transform_precoding, {rx_ports}}}, {"symbols"}, {"estimates", {subc, symbols, rx, layers}}, ...
ENTRY = re.compile(
    r"\{\{\s*([-0-9.eE+]+),\s*([-0-9.eE+]+),\s*\{\s*(\d+),\s*\{\{?([01,\s]*)\}?\},\s*modulation_scheme::(\w+),\s*(\d+),\s*(\d+),"
    r"\s*\{([01,\s]*)\},\s*dmrs_type::TYPE(\d),\s*(\d+),\s*(\d+),\s*(\d+),\s*(true|false),\s*\{([\d,\s]*)\}\}\},"
    r"\s*\{\"[^\"]*\"\},\s*\{\"[^\"]*\",\s*\{([\d,\s]*)\}\}")


def ints(text):
    return [int(x) for x in re.findall(r"\d+", text)]


def extract(reference_root):
    text = open(os.path.join(reference_root, HEADER)).read()
    out = []
    for m in ENTRY.finditer(text):
        rb = ints(m.group(4))
        dims = ints(m.group(15))
        out.append({
            "noise_var": float(m.group(1)),
            "rnti": int(m.group(3)),
            "rb_mask": [i for i, b in enumerate(rb) if b],
            "nof_rb": len(rb),
            "modulation": m.group(5),
            "start_symbol_index": int(m.group(6)),
            "nof_symbols": int(m.group(7)),
            "dmrs_symbols": [i for i, b in enumerate(ints(m.group(8))) if b],
            "dmrs_type": int(m.group(9)),
            "nof_cdm_groups_without_data": int(m.group(10)),
            "n_id": int(m.group(11)),
            "nof_tx_layers": int(m.group(12)),
            "transform_precoding": m.group(13) == "true",
            "rx_ports": ints(m.group(14)),
            "estimate_dims": {"subcarrier": dims[0], "symbol": dims[1], "rx_port": dims[2], "tx_layer": dims[3]},
        })
    return out


def render(configs):
    return "[\n" + ",\n".join(json.dumps(c, sort_keys=False) for c in configs) + "\n]\n"


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/srsRAN-5G-ER"
    dst = sys.argv[2] if len(sys.argv) > 2 else OUTPUT
    configs = extract(root)
    open(dst, "w").write(render(configs))
    print("%d configurations -> %s" % (len(configs), dst))
