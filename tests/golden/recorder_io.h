// What the golden recorders (record_*_reference.cpp) share and that needs nothing of the reference: .npy files, the seeded
// 32-bit finaliser, bf16 rounding, and the readers and writers for the flat JSON of the *_configs.json files.  Standard library
// only; tests/recorder_io_check.cpp checks it on the CPU, without a reference.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <regex>
#include <sstream>
#include <string>
#include <vector>

// One array as .npy, version 1.0: `descr` is NumPy's ("<i8", "|u1", "<c8", ...), the shape (n,) for cols == 0 and
// (n / cols, cols) otherwise, the header padded with spaces so that the data starts at a multiple of 64 bytes.
template <typename T>
inline void write_npy(const std::string& path, const char* descr, const std::vector<T>& data, size_t cols = 0)
{
  std::ostringstream shape;
  if (cols == 0) {
    shape << "(" << data.size() << ",)";
  } else {
    shape << "(" << data.size() / cols << ", " << cols << ")";
  }
  std::string header = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': " + shape.str() + ", }";
  while ((10 + header.size() + 1) % 64 != 0) {
    header += ' ';
  }
  header += '\n';
  std::ofstream  f(path, std::ios::binary);
  const char     magic[8] = {'\x93', 'N', 'U', 'M', 'P', 'Y', 1, 0};
  const uint16_t len      = (uint16_t)header.size();
  f.write(magic, 8);
  f.write((const char*)&len, 2);
  f.write(header.data(), header.size());
  f.write((const char*)data.data(), data.size() * sizeof(T));
}
inline void write_npy(const std::string& path, const std::vector<uint8_t>& data)
{
  write_npy(path, "|u1", data, 0);
}

// The data of a version 1.0 .npy file of 32-bit words, whatever its shape.
inline std::vector<uint32_t> read_npy_u32(const std::string& path)
{
  std::ifstream f(path, std::ios::binary);
  char          head[10];
  f.read(head, 10);
  const unsigned len = (unsigned char)head[8] | ((unsigned char)head[9] << 8);
  f.seekg(10 + len);
  std::vector<char>     bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<uint32_t> out(bytes.size() / 4);
  if (!out.empty()) { // (memcpy takes no null pointer, and an empty vector may hold one)
    std::memcpy(out.data(), bytes.data(), out.size() * 4);
  }
  return out;
}

// The 32-bit finaliser behind every seeded input that is not stored.
inline uint32_t mix(uint32_t h)
{
  h ^= h >> 16;
  h *= 0x85EBCA6BU;
  h ^= h >> 13;
  h *= 0xC2B2AE35U;
  h ^= h >> 16;
  return h;
}

inline uint32_t bf16_bits(float v) // nearest, ties to even
{
  uint32_t u;
  std::memcpy(&u, &v, 4);
  return (u + 0x7FFFU + ((u >> 16) & 1U)) >> 16;
}
inline float bf16_value(uint32_t bits)
{
  const uint32_t u = bits << 16;
  float          v;
  std::memcpy(&v, &u, 4);
  return v;
}

// ---- fields of one flat JSON object, by regular expression: `"key": value` as Python's json.dump writes it ----

// An integer that must be there.
inline int json_int(const std::string& obj, const char* key)
{
  std::smatch m;
  if (!std::regex_search(obj, m, std::regex(std::string("\"") + key + "\": (-?[0-9]+)"))) {
    std::fprintf(stderr, "no %s\n", key);
    std::exit(1);
  }
  return std::stoi(m[1]);
}
// An integer that may be missing or null (`none` then), or a boolean (1, 0).
inline int json_int(const std::string& obj, const char* key, int none)
{
  std::smatch m;
  if (!std::regex_search(obj, m, std::regex(std::string("\"") + key + "\": (-?[0-9]+|null|true|false)"))) {
    return none;
  }
  const std::string v = m[1];
  return v == "null" ? none : v == "true" ? 1 : v == "false" ? 0 : std::stoi(v);
}
inline double json_float(const std::string& obj, const char* key)
{
  std::smatch m;
  if (!std::regex_search(obj, m, std::regex(std::string("\"") + key + "\": (-?[0-9.eE+-]+)"))) {
    std::fprintf(stderr, "no %s\n", key);
    std::exit(1);
  }
  return std::stod(m[1]);
}
// A list of non-negative integers, empty where the key is missing.  `chars` is the character class a list is made of: a file
// written with an indent has line breaks inside its lists ("0-9, \n").
inline std::vector<int> json_list(const std::string& obj, const char* key, const char* chars = "0-9, ")
{
  std::smatch      m;
  std::vector<int> out;
  if (std::regex_search(obj, m, std::regex(std::string("\"") + key + "\": \\[([" + chars + "]*)\\]"))) {
    std::stringstream s(std::regex_replace(m[1].str(), std::regex(","), " "));
    for (int v; s >> v;) {
      out.push_back(v);
    }
  }
  return out;
}
// A number or a string as text, without its quotes.
inline std::string json_field(const std::string& obj, const char* key)
{
  std::smatch m;
  if (!std::regex_search(obj, m, std::regex(std::string("\"") + key + "\": \"?([^\",}]+)"))) {
    std::fprintf(stderr, "no %s\n", key);
    std::exit(1);
  }
  return m[1];
}

// [1, 2, 3], as json.dump writes a list.
inline std::string list_json(const std::vector<int>& v)
{
  std::string s = "[";
  for (size_t i = 0; i != v.size(); ++i) {
    s += (i ? ", " : "") + std::to_string(v[i]);
  }
  return s + "]";
}

// first, first + 1, ..., first + count - 1
inline std::vector<int> range(int first, int count)
{
  std::vector<int> v;
  for (int i = 0; i != count; ++i) {
    v.push_back(first + i);
  }
  return v;
}
