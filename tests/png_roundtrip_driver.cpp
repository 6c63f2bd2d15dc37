// Round trip of host/png_writer.hpp through host/png_reader.hpp (tests/test_camera_maps_restatement.py compiles and runs this,
// once plainly and once with -fsanitize=address,undefined, and reads the files it leaves with PIL).
//   png_roundtrip_driver <directory>
// writes <directory>/<gray|rgb>_<w>x<h>.png with pixel (x, y, c) = (7 x + 13 y + 29 c + (x y) mod 251) mod 256.
#include <cstdio>
#include <string>
#include <vector>

#include "host/png_reader.hpp"
#include "host/png_writer.hpp"

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: png_roundtrip_driver <directory>\n"); return 2; }
  const int sizes[3][2] = {{1, 1}, {67, 5}, {960, 540}};
  for (const auto& s : sizes) {
    for (int ch : {1, 3}) {
      const int w = s[0], h = s[1];
      std::vector<uint8_t> px(size_t(w) * h * ch);
      for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
          for (int c = 0; c < ch; ++c) px[(size_t(y) * w + x) * ch + c] = uint8_t((7 * x + 13 * y + 29 * c + (x * y) % 251) % 256);
      const std::string path = std::string(argv[1]) + "/" + (ch == 1 ? "gray_" : "rgb_") + std::to_string(w) + "x" + std::to_string(h) + ".png";
      std::string err;
      if (!oicc_png::write_png(path, w, h, ch, px.data(), &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
      oicc_png::Image img;
      if (!oicc_png::read_png(path, &img, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
      if (img.width != w || img.height != h || img.channels != ch || img.pixels != px) { std::fprintf(stderr, "%s: round trip differs\n", path.c_str()); return 1; }
    }
  }
  std::string err;
  const uint8_t one = 0;
  if (oicc_png::write_png(std::string(argv[1]) + "/bad.png", 1, 1, 2, &one, &err)) { std::fprintf(stderr, "two channels were accepted\n"); return 1; }
  std::printf("png round trip ok\n");
  return 0;
}
