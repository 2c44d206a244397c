"""Writes the UCI decoder fixtures from a checkout of srsRAN-5G-ER, settings and table numbers only:

  uci_decoder_configs.json  the entries of tests/unittests/phy/upper/channel_processors/uci/uci_decoder_test_data.h: message
                            length, LLR length and modulation.  The tests' vector files are not used: the recorded inputs and
                            answers of tests/golden/uci_reference.npz come from record_uci_reference.cpp.
  uci_tables.json           the numbers of TS 38.212 Table 5.3.3.3-1, the eleven basis sequences of the (32, K) block code
                            (lib/phy/upper/channel_coding/short/short_block_encoder_impl.cpp), row k holding M_{i,k}, i = 0..31,
                            and the eleven detection thresholds of short_block_detector_impl.cpp.

    python tests/golden/extract_uci_configs.py [REFERENCE_ROOT] [OUTPUT_DIR]
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TEST_DATA = os.path.join("tests", "unittests", "phy", "upper", "channel_processors", "uci", "uci_decoder_test_data.h")
SHORT_ENCODER = os.path.join("lib", "phy", "upper", "channel_coding", "short", "short_block_encoder_impl.cpp")
SHORT_DETECTOR = os.path.join("lib", "phy", "upper", "channel_coding", "short", "short_block_detector_impl.cpp")

CASE = re.compile(r"\{(\d+), (\d+), \{modulation_scheme::(\w+)\}, \{\"")


def configs(reference_root):
    text = open(os.path.join(reference_root, TEST_DATA)).read()
    return [{"message_length": int(a), "llr_length": int(e), "modulation": m} for a, e, m in CASE.findall(text)]


def tables(reference_root):
    text = open(os.path.join(reference_root, SHORT_ENCODER)).read()
    body = text[text.index("BASIS_SEQUENCES = {"):text.index("static void validate_spans")]
    rows = [[int(x) for x in re.findall(r"\d", row)] for row in re.findall(r"\{([01, ]+)\}", body)]
    assert len(rows) == 11 and all(len(r) == 32 for r in rows)
    text = open(os.path.join(reference_root, SHORT_DETECTOR)).read()
    thresholds = [int(x) for x in re.search(r"THRESHOLDS = \{([0-9, ]+)\}", text).group(1).split(",")]
    assert len(thresholds) == 11
    return {"basis": rows, "thresholds": [thresholds]}


def render(items):
    return "[\n" + ",\n".join(json.dumps(c, sort_keys=False) for c in items) + "\n]\n"


def render_tables(t):
    return "{\n" + ",\n".join('"%s": [\n%s\n]' % (k, ",\n".join(json.dumps(r) for r in v)) for k, v in t.items()) + "\n}\n"


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SRSRAN_ROOT", "srsRAN-5G-ER")
    dst = sys.argv[2] if len(sys.argv) > 2 else HERE
    c, t = configs(root), tables(root)
    open(os.path.join(dst, "uci_decoder_configs.json"), "w").write(render(c))
    open(os.path.join(dst, "uci_tables.json"), "w").write(render_tables(t))
    print("%d configurations, %d basis sequences -> %s" % (len(c), len(t["basis"]), dst))
