"""Writes prach_demod_configs.json from a checkout of srsRAN-5G-ER, settings only: the entries of
tests/unittests/phy/lower/modulation/ofdm_prach_demodulator_test_data.h -- sampling rate and
ofdm_prach_demodulator::configuration (format, time- and frequency-domain occasions, start symbol, RB offset, grid size, PUSCH
spacing).  The test's vector files are not used: tests/golden/record_prach_demod_reference.cpp records the reference's answers
on seeded inputs instead.

    python tests/golden/extract_prach_demod_configs.py [REFERENCE_ROOT] [OUTPUT_DIR]
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TEST_DATA = os.path.join("tests", "unittests", "phy", "lower", "modulation", "ofdm_prach_demodulator_test_data.h")
CASE = re.compile(r"\{\{sampling_rate::from_MHz\(([0-9.]+)\),\s*\{to_prach_format_type\(\"([^\"]+)\"\),\s*(\d+),\s*(\d+),\s*(\d+),"
                  r"\s*(\d+),\s*(\d+),\s*subcarrier_spacing::kHz(\d+)\}\}")


def configs(reference_root):
    text = open(os.path.join(reference_root, TEST_DATA)).read()
    out = []
    for m in CASE.finditer(text):
        out.append({"srate_hz": int(round(float(m.group(1)) * 1e6)), "format": m.group(2), "nof_td_occasions": int(m.group(3)),
                    "nof_fd_occasions": int(m.group(4)), "start_symbol": int(m.group(5)), "rb_offset": int(m.group(6)),
                    "nof_prb_ul_grid": int(m.group(7)), "pusch_scs_kHz": int(m.group(8))})
    return out


def render(items):
    return "[\n" + ",\n".join(json.dumps(c, sort_keys=False) for c in items) + "\n]\n"


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SRSRAN_ROOT", "srsRAN-5G-ER")
    dst = sys.argv[2] if len(sys.argv) > 2 else HERE
    items = configs(root)
    open(os.path.join(dst, "prach_demod_configs.json"), "w").write(render(items))
    print("%d entries -> %s" % (len(items), os.path.join(dst, "prach_demod_configs.json")))
