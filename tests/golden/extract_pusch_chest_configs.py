"""Writes tests/golden/pusch_chest_configs.json: the 96 configurations of the reference's PUSCH DM-RS estimator unit test
(tests/unittests/phy/upper/signal_processors/dmrs_pusch_estimator_test_data.h of srsRAN-5G-ER), settings only.  The test's
vector files are not used: tests/test_pusch_channel_estimator.py builds grids of its own for these configurations.
`slot` is {numerology, sfn, subframe, slot}; slot_index = subframe * 2^numerology + slot.

    python tests/golden/extract_pusch_chest_configs.py [REFERENCE_ROOT] [OUTPUT]
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join("tests", "unittests", "phy", "upper", "signal_processors", "dmrs_pusch_estimator_test_data.h")
OUTPUT = os.path.join(HERE, "pusch_chest_configs.json")

# {test_label::L, {{numerology, sfn, subframe, slot}, dmrs_type::TYPEn, scrambling_id, n_scid, scaling, cyclic_prefix::CP,
#   {symbols_mask}, {rb_mask}, first_symbol, nof_symbols, nof_tx_layers, {rx_ports}}, est_noise_var, est_rsrp, ...
ENTRY = re.compile(
    r"\{test_label::(\w+),\s*\{\{\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+)\s*\},\s*dmrs_type::TYPE(\d),\s*(\d+),\s*(\d+),"
    r"\s*([-0-9.eE+]+),\s*cyclic_prefix::(\w+),\s*\{([01,\s]*)\},\s*\{([01,\s]*)\},\s*(\d+),\s*(\d+),\s*(\d+),"
    r"\s*\{([\d,\s]*)\}\},\s*([-0-9.eE+]+),\s*([-0-9.eE+]+),")


def ints(text):
    return [int(x) for x in re.findall(r"\d+", text)]


def extract(reference_root):
    text = open(os.path.join(reference_root, HEADER)).read()
    out = []
    for m in ENTRY.finditer(text):
        mu, sf, slot = int(m.group(2)), int(m.group(4)), int(m.group(5))
        rb = ints(m.group(12))
        out.append({
            "label": m.group(1),
            "slot": [mu, int(m.group(3)), sf, slot],
            "numerology": mu,
            "slot_index": sf * (1 << mu) + slot,
            "dmrs_type": int(m.group(6)),
            "scrambling_id": int(m.group(7)),
            "n_scid": int(m.group(8)),
            "scaling": float(m.group(9)),
            "cyclic_prefix": m.group(10),
            "dmrs_symbols": [i for i, b in enumerate(ints(m.group(11))) if b],
            "rb_mask": [i for i, b in enumerate(rb) if b],
            "nof_rb": len(rb),
            "first_symbol": int(m.group(13)),
            "nof_symbols": int(m.group(14)),
            "nof_tx_layers": int(m.group(15)),
            "rx_ports": ints(m.group(16)),
            "est_noise_var": float(m.group(17)),
            "est_rsrp": float(m.group(18)),
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
