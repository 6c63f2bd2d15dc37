// Minimal PNG reader over zlib for extract_board_to_json: 8-bit gray (colour type 0), gray + alpha (4), RGB (2) and
// RGBA (6), non-interlaced, every row filter (None, Sub, Up, Average, Paeth; PNG specification section 9).  Anything
// else (palette, 1/2/4/16-bit samples, Adam7 interlacing) is an error.  Pixels come back in the file's channel layout.
#pragma once
#include <zlib.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

namespace oicc_png {

struct Image {
  int width = 0, height = 0, channels = 0;   // channels 1 (gray), 2 (gray + alpha), 3 (RGB), 4 (RGBA)
  std::vector<uint8_t> pixels;               // [height][width][channels]
};

inline uint32_t be32(const uint8_t* p) { return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | uint32_t(p[3]); }

inline bool read_png(const std::string& path, Image* out, std::string* err) {
  auto fail = [&](const std::string& m) { *err = path + ": " + m; return false; };
  std::ifstream f(path, std::ios::binary);
  if (!f) return fail("cannot open");
  const std::vector<uint8_t> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  static const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
  if (b.size() < 8 || std::memcmp(b.data(), sig, 8) != 0) return fail("not a PNG file");
  size_t pos = 8;
  int w = 0, h = 0, ch = 0;
  bool have_header = false, ended = false;
  std::vector<uint8_t> idat;
  while (pos + 12 <= b.size()) {
    const uint32_t len = be32(&b[pos]);
    if (len > b.size() - pos - 12) return fail("truncated chunk");
    const std::string type(reinterpret_cast<const char*>(&b[pos + 4]), 4);
    const uint8_t* d = &b[pos + 8];
    if (type == "IHDR") {
      if (len != 13) return fail("bad IHDR");
      w = int(be32(d)); h = int(be32(d + 4));
      const int depth = d[8], ctype = d[9], interlace = d[12];
      if (depth != 8) return fail("unsupported bit depth " + std::to_string(depth) + " (8-bit samples only)");
      if (interlace != 0) return fail("interlaced PNGs are not supported");
      if (d[10] != 0 || d[11] != 0) return fail("unknown compression or filter method");
      switch (ctype) { case 0: ch = 1; break; case 4: ch = 2; break; case 2: ch = 3; break; case 6: ch = 4; break;
        default: return fail("unsupported colour type " + std::to_string(ctype) + " (gray, gray + alpha, RGB, RGBA only)"); }
      if (w <= 0 || h <= 0 || int64_t(w) * h > (int64_t(1) << 28)) return fail("bad image size");
      have_header = true;
    } else if (type == "IDAT") {
      idat.insert(idat.end(), d, d + len);
    } else if (type == "IEND") {
      ended = true; break;
    }
    pos += size_t(len) + 12;
  }
  if (!have_header || !ended || idat.empty()) return fail("missing IHDR, IDAT or IEND");
  const size_t stride = size_t(w) * size_t(ch);
  std::vector<uint8_t> raw((stride + 1) * size_t(h));
  uLongf n = uLongf(raw.size());
  if (uncompress(raw.data(), &n, idat.data(), uLong(idat.size())) != Z_OK || n != raw.size()) return fail("bad image data");
  out->width = w; out->height = h; out->channels = ch;
  out->pixels.assign(stride * size_t(h), 0);
  for (int y = 0; y < h; ++y) {
    const uint8_t ft = raw[size_t(y) * (stride + 1)];
    const uint8_t* s = &raw[size_t(y) * (stride + 1) + 1];
    uint8_t* o = &out->pixels[size_t(y) * stride];
    const uint8_t* up = y > 0 ? o - stride : nullptr;
    for (size_t x = 0; x < stride; ++x) {
      const int a = x >= size_t(ch) ? o[x - size_t(ch)] : 0, c = (up && x >= size_t(ch)) ? up[x - size_t(ch)] : 0, u = up ? up[x] : 0;
      int v = s[x];
      switch (ft) {
        case 0: break;
        case 1: v += a; break;
        case 2: v += u; break;
        case 3: v += (a + u) >> 1; break;
        case 4: {
          const int p = a + u - c, pa = std::abs(p - a), pb = std::abs(p - u), pc = std::abs(p - c);
          v += (pa <= pb && pa <= pc) ? a : (pb <= pc ? u : c);
          break; }
        default: return fail("bad row filter " + std::to_string(ft));
      }
      o[x] = uint8_t(v);
    }
  }
  return true;
}

}  // namespace oicc_png
