"""Writes the two PRACH fixtures from a checkout of srsRAN-5G-ER, settings and recorded results only:

  prach_thresholds.json        the rows of lib/phy/upper/channel_processors/prach_detector_generic_thresholds.h
                               (ports, scs, format, zcz, threshold, margin, flag); the closing sentinel row of format
                               `invalid` is not a row of the table and is left out.
  prach_detector_configs.json  the entries of tests/unittests/phy/upper/channel_processors/prach_detector_test_data.h:
                               the configuration, true_delay and the expected preamble index, time advance and metric.
                               The test's vector files are not used: tests/test_prach_detector.py builds its own buffers.

    python tests/golden/extract_prach_configs.py [REFERENCE_ROOT] [OUTPUT_DIR]
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
THRESHOLDS = os.path.join("lib", "phy", "upper", "channel_processors", "prach_detector_generic_thresholds.h")
TEST_DATA = os.path.join("tests", "unittests", "phy", "upper", "channel_processors", "prach_detector_test_data.h")

FORMATS = ["0", "1", "2", "3", "A1", "A2", "A3", "B1", "B4", "C0", "C2", "A1/B1", "A2/B2", "A3/B3"]
FORMAT_ENUM = {"zero": "0", "one": "1", "two": "2", "three": "3", "A1_B1": "A1/B1", "A2_B2": "A2/B2", "A3_B3": "A3/B3"}
SCS_ENUM = {"kHz15": "15", "kHz30": "30", "kHz60": "60", "kHz120": "120", "kHz1_25": "1.25", "kHz5": "5"}

ROW = re.compile(r"^\s*\{\{/\* nof_rx_ports \*/\s*(\d+),\s*prach_subcarrier_spacing::(\w+),\s*prach_format_type::(\w+),"
                 r"\s*/\* ZCZ \*/\s*(\d+),\s*/\* combine symbols \*/\s*(\w+)\},\s*\{([0-9.]+)F,\s*(\d+)\},\s*th_flag::(\w+)\},",
                 re.M)
NUM = r"([-0-9.eE+]+)"
CASE = re.compile(r"\{\{\{(\d+),\s*to_prach_format_type\(\"([^\"]+)\"\),\s*restricted_set_config::(\w+),\s*(\d+),\s*(\d+),\s*(\d+),"
                  r"\s*to_ra_subcarrier_spacing\(\"([0-9.]+)kHz\"\),\s*(\d+)\},\s*phy_time_unit::from_seconds\(" + NUM + r"\),"
                  r"\s*\{" + NUM + r",\s*phy_time_unit::from_seconds\(" + NUM + r"\),\s*phy_time_unit::from_seconds\(" + NUM + r"\),"
                  r"\s*\{\{(\d+),\s*phy_time_unit::from_seconds\(" + NUM + r"\),\s*" + NUM + r"\}\}\}\}")


def thresholds(reference_root):
    text = open(os.path.join(reference_root, THRESHOLDS)).read()
    rows = []
    for m in ROW.finditer(text):
        if m.group(3) == "invalid":
            continue
        assert m.group(5) == "true"
        rows.append({"ports": int(m.group(1)), "scs": SCS_ENUM[m.group(2)], "format": FORMAT_ENUM.get(m.group(3), m.group(3)),
                     "zcz": int(m.group(4)), "threshold": m.group(6), "margin": int(m.group(7)), "flag": m.group(8)})
    return rows


def configs(reference_root):
    text = open(os.path.join(reference_root, TEST_DATA)).read()
    out = []
    for m in CASE.finditer(text):
        out.append({"root_sequence_index": int(m.group(1)), "format": m.group(2), "restricted_set": m.group(3),
                    "zero_correlation_zone": int(m.group(4)), "start_preamble_index": int(m.group(5)),
                    "nof_preamble_indices": int(m.group(6)), "ra_scs": "%g" % float(m.group(7)), "nof_rx_ports": int(m.group(8)),
                    "true_delay": float(m.group(9)), "rssi_dB": float(m.group(10)), "preamble_index": int(m.group(13)),
                    "time_advance": float(m.group(14)), "detection_metric": float(m.group(15))})
    return out


def render(items):
    return "[\n" + ",\n".join(json.dumps(c, sort_keys=False) for c in items) + "\n]\n"


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SRSRAN_ROOT", "srsRAN-5G-ER")
    dst = sys.argv[2] if len(sys.argv) > 2 else HERE
    for name, items in (("prach_thresholds.json", thresholds(root)), ("prach_detector_configs.json", configs(root))):
        open(os.path.join(dst, name), "w").write(render(items))
        print("%d entries -> %s" % (len(items), os.path.join(dst, name)))
