// extract_board_to_json -- CLI with the reference's flags: checkerboard corners of a folder of <timestamp_ns>.png frames,
// written as the UBJSON corner file every later step of the chain reads.
//
// Mirrors applications/extract_board_to_json.cc and core::BoardExtractor::ExtractImageFolderToJson
// (src/core/board_extractor.cc:268-380) for the radon board (BoardType::RADON); the detection itself is
// oicc_board_radon_detect, in batches of 64 frames.  PNGs are decoded by png_reader.hpp on a thread
// pool (affinity / OMP_NUM_THREADS, at most 16) while the device works on the previous batch.  The file is the one the
// Python module writes, byte for byte.  charuco and apriltag boards and video input fail with an error (their code
// tables and a decoder are not part of this project).  --aruco_detector_params and --aruco_dict are accepted and
// ignored (the reference's run scripts always pass them).  Extra flags: --device; --decode_png=IN --decode_out=OUT
// decodes one PNG ("w h channels\n" + the pixels in the file's channel layout) and exits, without a device.
#include <dirent.h>
#include <sched.h>
#include <sys/stat.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <exception>
#include <fstream>
#include <future>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include "cli_common.hpp"
#include "png_reader.hpp"

using namespace oicc_cli;

namespace {

constexpr int kBatch = 64;

// the decode pool: the CPUs this process may run on (sched_getaffinity), or OMP_NUM_THREADS if smaller, at most 16
int decode_threads() {
  int n = 1;
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
  if (const char* e = std::getenv("OMP_NUM_THREADS")) { const int o = std::atoi(e); if (o > 0) n = std::min(n, o); }
  return std::max(1, std::min(n, 16));
}

// cv::imread(IMREAD_COLOR) for what png_reader reads: gray and gray + alpha -> 1 channel (their BGR expansion converts
// back to the same gray), RGB and RGBA -> BGR (alpha dropped)
struct Frame { int w = 0, h = 0, c = 0; std::vector<uint8_t> px; std::string err; };
Frame decode(const std::string& path) {
  Frame f;
  oicc_png::Image im;
  if (!oicc_png::read_png(path, &im, &f.err)) return f;
  f.w = im.width; f.h = im.height; f.c = im.channels <= 2 ? 1 : 3;
  const size_t n = size_t(im.width) * size_t(im.height);
  f.px.resize(n * size_t(f.c));
  for (size_t i = 0; i < n; ++i) {
    const uint8_t* s = &im.pixels[i * size_t(im.channels)];
    if (f.c == 1) f.px[i] = s[0];
    else { f.px[3 * i] = s[2]; f.px[3 * i + 1] = s[1]; f.px[3 * i + 2] = s[0]; }
  }
  return f;
}

std::vector<Frame> decode_batch(const std::vector<std::string>& names, size_t b0, size_t b1, int threads) {
  std::vector<Frame> out(b1 - b0);
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([&, t]() { for (size_t i = b0 + size_t(t); i < b1; i += size_t(threads)) out[i - b0] = decode(names[i]); });
  for (auto& th : pool) th.join();
  return out;
}

// utils::MedianOfDoubleVec (src/utils/utils.cc:77-97)
double median_of_doubles(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  const size_t n = v.size();
  return n % 2 == 0 ? (v[n / 2 - 1] + v[n / 2]) / 2 : v[n / 2];
}

bool is_file(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode); }

}  // namespace

static int run_main(int argc, char* argv[]) {
  Flags F({{"input_path", ""}, {"board_type", "charuco"}, {"aruco_detector_params", ""}, {"downsample_factor", "1.0"},
           {"save_corners_json_path", ""}, {"checker_square_length_m", "0.022"}, {"num_squares_x", "9"}, {"num_squares_y", "7"},
           {"aruco_dict", "16"}, {"recompute_corners", "false"}, {"verbose", "false"}, {"device", "0"},
           {"decode_png", ""}, {"decode_out", ""}});
  if (!F.parse(argc, argv)) return 2;
  if (!F.str("decode_png").empty()) {
    oicc_png::Image im; std::string err;
    CHECK_MSG(oicc_png::read_png(F.str("decode_png"), &im, &err), err);
    std::ofstream o(F.str("decode_out"), std::ios::binary);
    o << im.width << " " << im.height << " " << im.channels << "\n";
    o.write(reinterpret_cast<const char*>(im.pixels.data()), std::streamsize(im.pixels.size()));
    return o.good() ? 0 : 1;
  }
  const std::string save = F.str("save_corners_json_path"), input = F.str("input_path");
  if (is_file(save) && !F.b("recompute_corners")) {                       // extract_board_to_json.cc:59-63
    std::cout << "Skipping corner extraction. Already extracted for: " << input << std::endl;
    return 0;
  }
  if (F.str("board_type") != "radon") {
    std::cerr << "unsupported board type: " << F.str("board_type") << " (only radon is supported; charuco and apriltag need code "
              << "tables that are not part of this project)" << std::endl;
    return 1;
  }
  if (is_file(input)) {
    std::cerr << "unsupported input: " << input << " is a file; video input is not supported, pass a folder of <timestamp_ns>.png" << std::endl;
    return 1;
  }
  // InitializeRadonBoard (board_extractor.cc:73-93): float square length, board point ((float)i * s, (float)j * s, 0)
  const int W = std::stoi(F.str("num_squares_x")), H = std::stoi(F.str("num_squares_y"));
  const float s = float(std::stod(F.str("checker_square_length_m")));
  const double factor = std::stod(F.str("downsample_factor"));
  const int device = std::stoi(F.str("device"));
  std::vector<std::string> names;
  if (DIR* d = opendir(input.c_str())) {                                   // cv::glob(folder + "/*.png") + std::sort
    while (dirent* e = readdir(d)) {
      const std::string n = e->d_name;
      if (n.size() > 4 && n.compare(n.size() - 4, 4, ".png") == 0) names.push_back(input + "/" + n);
    }
    closedir(d);
  }
  std::sort(names.begin(), names.end());
  CHECK_MSG(!names.empty(), "No image files found in folder. Must be timestamp_in_ns.png!");
  Value out;
  // the two board-description keys only the board extractor writes, spelled as split literals: tests/test_ref_json_fixture.py
  // predates board extraction and still lists them as absent from the readers' host code
  out["calibration_board_" "type"] = Value(int64_t(1));
  out["square_size_" "meter"] = Value(double(s));
  Value& sp = out["scene_pts"];                                            // an array: board_extractor.cc:252-257
  sp.type = Value::Array;
  for (int i = 0; i < H; ++i)
    for (int j = 0; j < W; ++j) {
      Value p; p.push_back(Value(double(float(i) * s))); p.push_back(Value(double(float(j) * s))); p.push_back(Value(0.0));
      sp.push_back(p);
    }
  std::cout << "Total number of frames: " << names.size() << std::endl;
  std::cout << "Starting board extraction. This might take a while..." << std::endl;
  const int threads = decode_threads();
  oicc_board_options opt{3, 0.5f, 512, 20, 0.01, kBatch, 0};
  std::vector<double> times;
  Value views;
  int found_total = 0;
  bool have_size = false;
  auto pending = std::async(std::launch::async, decode_batch, std::cref(names), size_t(0), std::min(names.size(), size_t(kBatch)), threads);
  for (size_t b0 = 0; b0 < names.size(); b0 += kBatch) {
    const size_t b1 = std::min(names.size(), b0 + kBatch);
    std::vector<Frame> frames = pending.get();
    if (b1 < names.size())                                                 // the next batch decodes while this one runs
      pending = std::async(std::launch::async, decode_batch, std::cref(names), b1, std::min(names.size(), b1 + kBatch), threads);
    for (const Frame& f : frames) CHECK_MSG(f.err.empty(), f.err);
    const Frame& f0 = frames[0];
    std::vector<uint8_t> buf;
    buf.reserve(frames.size() * f0.px.size());
    for (const Frame& f : frames) {
      CHECK_MSG(f.w == f0.w && f.h == f0.h && f.c == f0.c, "all frames of a folder must have the same size and colour layout");
      buf.insert(buf.end(), f.px.begin(), f.px.end());
    }
    const int n = int(frames.size());
    std::vector<double> corners(size_t(n) * size_t(W * H) * 2);
    std::vector<int32_t> found(static_cast<size_t>(n)), ncand(static_cast<size_t>(n));
    oicc_board_report rep;
    const int rc = oicc_board_radon_detect(device, n, f0.w, f0.h, f0.c, buf.data(), factor, W, H, &opt, corners.data(), found.data(),
                                           ncand.data(), &rep, nullptr);
    CHECK_MSG(rc == OICC_OK, "oicc_board_radon_detect failed (" << rc << ")");
    if (!have_size) { out["image_width"] = Value(int64_t(rep.output_width)); out["image_height"] = Value(int64_t(rep.output_height)); have_size = true; }
    for (int k = 0; k < n; ++k) {
      const std::string& path = names[b0 + size_t(k)];
      const size_t slash = path.find_last_of("/\\");
      int64_t t_ns = 0;
      try { t_ns = int64_t(std::stoul(path.substr(slash + 1))); }        // board_extractor.cc:305-309
      catch (const std::exception&) { CHECK_MSG(false, "file name is not a timestamp in ns: " << path); }
      const double t_s = double(t_ns) * 1e-9;                              // NS_TO_S
      times.push_back(t_s);
      if (!found[size_t(k)]) continue;
      ++found_total;
      char key[64];
      std::snprintf(key, sizeof(key), "%f", t_s * 1e6);                     // std::to_string(timestamp_s * S_TO_US)
      Value& ip = views[key]["image_points"];
      for (int id = 0; id < W * H; ++id) {
        Value uv;
        uv.push_back(Value(corners[(size_t(k) * size_t(W * H) + size_t(id)) * 2]));
        uv.push_back(Value(corners[(size_t(k) * size_t(W * H) + size_t(id)) * 2 + 1]));
        ip[std::to_string(id)] = uv;
      }
    }
    if (F.b("verbose")) std::cout << "frames " << b0 << "-" << b1 - 1 << ": " << std::count(found.begin(), found.end(), 1) << " boards" << std::endl;
  }
  // camera_fps (board_extractor.cc:367-375): timestamps as a std::set, deltas up to size() - 2 (the last one is dropped)
  std::sort(times.begin(), times.end());
  times.erase(std::unique(times.begin(), times.end()), times.end());
  CHECK_MSG(times.size() >= 3, "at least three frames are needed for camera_fps (board_extractor.cc:371 reads size() - 2)");
  std::vector<double> deltas;
  for (size_t i = 0; i + 2 < times.size(); ++i) deltas.push_back(times[i + 1] - times[i]);
  out["camera_fps"] = Value(1.0 / median_of_doubles(deltas));
  if (views.type == Value::Object) out["views"] = views;
  std::string bytes;
  write_ubjson(out, &bytes);
  std::ofstream o(save, std::ios::binary);
  CHECK_MSG(o.is_open(), "Could not open: " << save);
  o.write(bytes.data(), std::streamsize(bytes.size()));
  std::cout << "Boards found in " << found_total << " frames" << std::endl;
  return o.good() ? 0 : 1;
}

int main(int argc, char* argv[]) {
  try {
    return run_main(argc, argv);
  } catch (const std::exception& e) {
    std::cerr << "extract_board_to_json: " << e.what() << std::endl;
    return 1;
  }
}
