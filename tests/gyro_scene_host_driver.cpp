// Drives the host rules of the gyro warps (csrc/gyro_scene_host.h) without a device.  test_gyro_scene_host.py compiles it plain and
// with -fsanitize=address,undefined (both with -ffp-contract=off, as the library's units are) and compares what it prints with the
// numpy restatements:
//   gyro_scene_host_driver FILE     FILE holds "key count value ..." records, doubles as C99 hexadecimal floats (or inf / nan):
//     gyro_t [n], rates [n][3], q_i_c [4], frame_t [frames], scene = offset line_delay reference_row src_h   the scene
//     sigma [1]                                                   smoothing windows
//     accl_t [na], gravity_sigma [1]                              the horizon lock's decisions
//     z [frames], status [frames], zoom = mode window max_zoom    the applied zoom (over frame_t)
//     options [5], level_opts [5] with accl_t and accl [na][3], plan_q [frames][4] with plan_zoom [frames]     the argument checks
//   Every array is held in a vector of exactly its size, so that a read or write past an end is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>
#include "gyro_scene_host.h"

namespace {

using Record = std::map<std::string, std::vector<double>>;

bool read_records(const char* path, Record* out) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) return false;
  char key[64], tok[64];
  long count = 0;
  bool ok = true;
  while (ok && std::fscanf(f, "%63s %ld", key, &count) == 2) {
    std::vector<double>& v = (*out)[key];
    v.resize(size_t(count));
    for (long i = 0; i < count && ok; ++i) {
      ok = std::fscanf(f, "%63s", tok) == 1;
      if (ok) v[size_t(i)] = std::strtod(tok, nullptr);
    }
  }
  std::fclose(f);
  return ok;
}

void print(const char* name, const std::vector<double>& v) {
  std::printf("%s", name);
  for (double x : v) std::printf(" %a", x);
  std::printf("\n");
}

template <class T>
void print_int(const char* name, const std::vector<T>& v) {
  std::printf("%s", name);
  for (T x : v) std::printf(" %lld", static_cast<long long>(x));
  std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  using namespace oicc_rs;
  Record in;
  if (argc != 2 || !read_records(argv[1], &in)) { std::fprintf(stderr, "usage: gyro_scene_host_driver FILE\n"); return 2; }
  auto has = [&](const char* k) { return in.count(k) != 0; };
  const std::vector<double>&gyro_t = in["gyro_t"], &frame_t = in["frame_t"], &accl_t = in["accl_t"];
  const int64_t n = int64_t(gyro_t.size()), na = int64_t(accl_t.size());
  const int frames = int(frame_t.size());

  if (has("rates")) {
    std::vector<double> out(size_t(3 * n));
    rates_cam(n, in["rates"].data(), in["q_i_c"].data(), out.data());
    print("rates_cam", out);
  }
  if (has("q_i_c")) {
    std::vector<double> M(9);
    unit_rotation(in["q_i_c"].data(), M.data());
    print("Ric", M);
  }
  if (has("scene")) {
    const double offset = in["scene"][0], line_delay = in["scene"][1], reference_row = in["scene"][2];
    const double refd = reference_delay(reference_row, line_delay);
    std::vector<int64_t> first(size_t(frames), -7);
    std::vector<int32_t> count(size_t(frames), -7), status(size_t(frames), -7);
    frame_windows(n, gyro_t.data(), frames, frame_t.data(), offset, line_delay, reference_row, int(in["scene"][3]), first.data(), count.data(), status.data());
    print_int("first", first); print_int("count", count); print_int("status", status);

    std::vector<int64_t> interval(size_t(frames), -7);
    int path_first = 0, path_count = 0;
    const int rc = find_path(n, gyro_t.data(), frames, frame_t.data(), offset, refd, interval.data(), &path_first, &path_count);
    std::printf("path %d %d %d\n", rc, path_first, path_count);
    if (rc == OICC_OK) {
      print_int("interval", interval);
      if (has("sigma")) {
        std::vector<int32_t> lo(size_t(frames), -7), hi(size_t(frames), -7);
        smoothing_windows(frames, frame_t.data(), path_first, path_count, in["sigma"][0], lo.data(), hi.data());
        print_int("smooth_lo", lo); print_int("smooth_hi", hi);
      }
      if (has("gravity_sigma")) {
        std::vector<int32_t> frame_of(size_t(na), -7);
        std::vector<int64_t> sample_interval(size_t(na), -7), lo(size_t(frames), -7), hi(size_t(frames), -7);
        level_windows(n, gyro_t.data(), frames, frame_t.data(), offset, refd, na, accl_t.data(), in["gravity_sigma"][0], path_first, path_count,
                      frame_of.data(), sample_interval.data(), lo.data(), hi.data());
        print_int("frame_of", frame_of); print_int("sample_interval", sample_interval); print_int("level_lo", lo); print_int("level_hi", hi);
      }
    }
  }
  if (has("z")) {
    const oicc_stab_options o = {0.0, 0.0, int32_t(in["zoom"][0]), 0, in["zoom"][1], in["zoom"][2]};
    std::vector<int32_t> status(in["status"].begin(), in["status"].end());
    std::vector<double> Z(size_t(frames), -7.0);
    std::vector<uint8_t> clamped(size_t(frames), 7);
    applied_zoom(frames, frame_t.data(), in["z"].data(), status.data(), o, Z.data(), clamped.data());
    print("zoom", Z); print_int("clamped", clamped);
  }
  if (has("options")) {
    const std::vector<double>& v = in["options"];
    const oicc_stab_options o = {v[0], v[1], int32_t(v[2]), 0, v[3], v[4]};
    std::printf("options_ok %d %d\n", int(options_ok(&o)), int(options_ok(nullptr)));
  }
  if (has("level_opts")) {
    const std::vector<double>& v = in["level_opts"];
    const oicc_stab_level l = {na, accl_t.data(), in["accl"].data(), v[0], v[1], v[2], v[3], v[4]};
    std::printf("level_ok %d %d\n", int(level_ok(&l)), int(level_ok(nullptr)));
  }
  if (has("plan_q"))
    std::printf("plan_arrays_ok %d %d\n", int(plan_arrays_ok(in["plan_q"].data(), in["plan_zoom"].data(), int(in["plan_zoom"].size()))),
                int(plan_arrays_ok(nullptr, in["plan_zoom"].data(), int(in["plan_zoom"].size()))));
  return 0;
}
