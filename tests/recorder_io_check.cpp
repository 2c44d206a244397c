// Stand-alone driver of tests/golden/recorder_io.h for tests/test_recorder_io.py: no reference, no GPU.
//
//   recorder_io_check npy DIR            writes DIR/<dtype>_1d.npy (37), DIR/<dtype>_2d.npy (5 x 7), DIR/uint8_only.npy and
//                                        DIR/empty.npy, reads the uint32 and float32 ones back with read_npy_u32 and compares
//   recorder_io_check json FILE QUERY... prints one line per query over the text of FILE: int:KEY, opt:KEY:DEFAULT, float:KEY,
//                                        list:KEY, lines:KEY (a list with line breaks), field:KEY
//   recorder_io_check words IN OUT       IN: a .npy of uint32 words w.  Writes OUT/mix.npy (mix(w)), OUT/bits.npy (bf16_bits of
//                                        the float whose bits are w) and OUT/values.npy (bf16_value of those bits)
//   recorder_io_check text               prints list_json({}), list_json({7}), list_json(range(-2, 5))
#include "golden/recorder_io.h"

#include <type_traits>

namespace {

constexpr size_t N_1D = 37, ROWS = 5, COLS = 7;

// Value i: i * 37 mod 251, less 125 for a signed type (so within int8), plus (i mod 4) / 4 for a floating one.
template <typename T>
std::vector<T> values(size_t n)
{
  std::vector<T> v(n);
  for (size_t i = 0; i != n; ++i) {
    v[i] = (T)((long)(i * 37 % 251) - (std::is_signed<T>::value ? 125 : 0));
    if (std::is_floating_point<T>::value) {
      v[i] += (T)(i % 4) / (T)4;
    }
  }
  return v;
}

template <typename T>
void write_both(const std::string& dir, const char* name, const char* descr)
{
  write_npy(dir + "/" + name + "_1d.npy", descr, values<T>(N_1D)); // cols left out: the 1-D form
  write_npy(dir + "/" + name + "_2d.npy", descr, values<T>(ROWS * COLS), COLS);
}

int npy(const std::string& dir)
{
  write_both<int8_t>(dir, "int8", "|i1");
  write_both<uint8_t>(dir, "uint8", "|u1");
  write_both<int32_t>(dir, "int32", "<i4");
  write_both<int64_t>(dir, "int64", "<i8");
  write_both<uint32_t>(dir, "uint32", "<u4");
  write_both<float>(dir, "float32", "<f4");
  write_both<double>(dir, "float64", "<f8");
  write_npy(dir + "/uint8_only.npy", values<uint8_t>(N_1D)); // the form that takes no descr
  write_npy(dir + "/empty.npy", "<f4", std::vector<float>(), 0);

  // read_npy_u32 returns what write_npy wrote, whatever the shape.
  for (const char* name : {"uint32_1d", "uint32_2d", "float32_1d", "float32_2d", "empty"}) {
    const std::string           n    = name;
    const std::vector<uint32_t> back = read_npy_u32(dir + "/" + n + ".npy");
    std::vector<uint32_t>       want;
    if (n.rfind("uint32", 0) == 0) {
      want = values<uint32_t>(n == "uint32_1d" ? N_1D : ROWS * COLS);
    } else if (n != "empty") {
      const std::vector<float> f = values<float>(n == "float32_1d" ? N_1D : ROWS * COLS);
      want.resize(f.size());
      std::memcpy(want.data(), f.data(), 4 * f.size());
    }
    if (back != want) {
      std::printf("read_npy_u32(%s): %zu words, %zu expected, or other values\n", name, back.size(), want.size());
      return 1;
    }
  }
  std::printf("ok: npy\n");
  return 0;
}

int json(int argc, char** argv)
{
  std::ifstream     in(argv[2]);
  std::stringstream buffer;
  buffer << in.rdbuf();
  const std::string obj = buffer.str();
  for (int a = 3; a != argc; ++a) {
    const std::string q = argv[a], kind = q.substr(0, q.find(':'));
    std::string       key = q.substr(q.find(':') + 1);
    if (kind == "int") {
      std::printf("%d\n", json_int(obj, key.c_str()));
    } else if (kind == "opt") {
      const int none = std::stoi(key.substr(key.find(':') + 1));
      key            = key.substr(0, key.find(':'));
      std::printf("%d\n", json_int(obj, key.c_str(), none));
    } else if (kind == "float") {
      std::printf("%.17g\n", json_float(obj, key.c_str()));
    } else if (kind == "list") {
      std::printf("%s\n", list_json(json_list(obj, key.c_str())).c_str());
    } else if (kind == "lines") {
      std::printf("%s\n", list_json(json_list(obj, key.c_str(), "0-9, \n")).c_str());
    } else if (kind == "field") {
      std::printf("%s\n", json_field(obj, key.c_str()).c_str());
    } else {
      std::printf("unknown query %s\n", q.c_str());
      return 1;
    }
  }
  return 0;
}

int words(const std::string& in, const std::string& out)
{
  const std::vector<uint32_t> w = read_npy_u32(in);
  std::vector<uint32_t>       mixed(w.size()), bits(w.size());
  std::vector<float>          back(w.size());
  for (size_t i = 0; i != w.size(); ++i) {
    float f;
    std::memcpy(&f, &w[i], 4);
    mixed[i] = mix(w[i]);
    bits[i]  = bf16_bits(f);
    back[i]  = bf16_value(bits[i]);
  }
  write_npy(out + "/mix.npy", "<u4", mixed);
  write_npy(out + "/bits.npy", "<u4", bits);
  write_npy(out + "/values.npy", "<f4", back);
  std::printf("ok: %zu words\n", w.size());
  return 0;
}

} // namespace

int main(int argc, char** argv)
{
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "npy" && argc == 3) {
    return npy(argv[2]);
  }
  if (cmd == "json" && argc >= 3) {
    return json(argc, argv);
  }
  if (cmd == "words" && argc == 4) {
    return words(argv[2], argv[3]);
  }
  if (cmd == "text" && argc == 2) {
    std::printf("%s %s %s\n", list_json({}).c_str(), list_json({7}).c_str(), list_json(range(-2, 5)).c_str());
    return 0;
  }
  std::fprintf(stderr, "usage: %s npy DIR | json FILE QUERY... | words IN OUT | text\n", argv[0]);
  return 2;
}
