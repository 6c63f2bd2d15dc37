// Minimal PNG writer over zlib for undistort_images, the counterpart of png_reader.hpp: 8-bit gray (colour type 0) or RGB
// (colour type 2), non-interlaced, every row with filter type 0 (None), one IDAT chunk (PNG specification sections 5, 11).
#pragma once
#include <zlib.h>

#include <cstdint>
#include <fstream>
#include <string>
#include <vector>

namespace oicc_png {

inline void put_be32(std::vector<uint8_t>* out, uint32_t v) {
  out->push_back(uint8_t(v >> 24)); out->push_back(uint8_t(v >> 16)); out->push_back(uint8_t(v >> 8)); out->push_back(uint8_t(v));
}

// length, type, data, CRC-32 over type and data
inline void put_chunk(std::vector<uint8_t>* out, const char type[4], const uint8_t* data, size_t len) {
  put_be32(out, uint32_t(len));
  const size_t start = out->size();
  out->insert(out->end(), type, type + 4);
  if (len) out->insert(out->end(), data, data + len);
  put_be32(out, uint32_t(crc32(0L, out->data() + start, uInt(len + 4))));
}

// pixels [height][width][channels], channels 1 (gray) or 3 (RGB)
inline bool write_png(const std::string& path, int width, int height, int channels, const uint8_t* pixels, std::string* err) {
  auto fail = [&](const std::string& m) { *err = path + ": " + m; return false; };
  if (width <= 0 || height <= 0 || (channels != 1 && channels != 3) || !pixels) return fail("bad image (8-bit gray or RGB only)");
  if (int64_t(width) * height > (int64_t(1) << 28)) return fail("bad image size");
  const size_t stride = size_t(width) * size_t(channels);
  std::vector<uint8_t> raw((stride + 1) * size_t(height));
  for (int y = 0; y < height; ++y) {
    uint8_t* row = &raw[size_t(y) * (stride + 1)];
    row[0] = 0;                                               // filter type None
    for (size_t x = 0; x < stride; ++x) row[1 + x] = pixels[size_t(y) * stride + x];
  }
  uLongf n = compressBound(uLong(raw.size()));
  std::vector<uint8_t> packed(n);
  if (compress2(packed.data(), &n, raw.data(), uLong(raw.size()), 6) != Z_OK) return fail("compression failed");
  std::vector<uint8_t> out = {137, 80, 78, 71, 13, 10, 26, 10};
  std::vector<uint8_t> header;
  put_be32(&header, uint32_t(width)); put_be32(&header, uint32_t(height));
  header.push_back(8); header.push_back(channels == 1 ? 0 : 2);    // bit depth, colour type
  header.push_back(0); header.push_back(0); header.push_back(0);    // compression, filter method, no interlace
  put_chunk(&out, "IHDR", header.data(), header.size());
  put_chunk(&out, "IDAT", packed.data(), size_t(n));
  put_chunk(&out, "IEND", nullptr, 0);
  std::ofstream f(path, std::ios::binary);
  if (!f) return fail("cannot open for writing");
  f.write(reinterpret_cast<const char*>(out.data()), std::streamsize(out.size()));
  f.close();
  if (!f) return fail("write failed");
  return true;
}

}  // namespace oicc_png
