// tmc3_main.cpp -- CLI with the reference's surface (tmc3 <x>=<in.ply> <y>=<out.ply>,
// /root/reference/tmc3/TMC3.cpp:202-229, my_function.cpp:147-178) running the
// hot path on the GPU through the legacy adapter.  Flow kept as in main():
// read (scale 1000, trunc) -> bbox shift to >= 0 (buildingSeg ctor,
// TMC3.cpp:55-73) -> get_Normal_and_K_neighbor<15> -> seg_plane::get_planes ->
// set_plane_color -> write (scale 1.0, zero offset, binary).
#include <cstdio>
#include <limits>
#include <string>

#include "bs_legacy.hpp"
#include "bs_ply.hpp"

using Cloud = bs::PointSet3;
using VecD = bs::Vec3<double>;
using VecI = bs::Vec3<int>;
using VecC = bs::Vec3<uint16_t>;

static std::string after_equals(const char* arg)  // Split(path, "=")[1], my_function.cpp:167-172
{
  std::string s(arg);
  size_t p = s.find('=');
  return p == std::string::npos ? s : s.substr(p + 1);
}

int main(int argc, char* argv[])
{
  if (argc < 3) {
    fprintf(stderr, "usage: %s <x>=<in.ply> <y>=<out.ply> [--raster=<png prefix>] [--footprints=<file.obj>] [--buildings=<file.obj>]\n", argv[0]);
    return 2;
  }
  const std::string in = after_equals(argv[1]), out = after_equals(argv[2]);
  Cloud cloud;
  std::string err;
  if (!bs::ply::read(in, 1000.0, cloud, &err)) {
    fprintf(stderr, "ply read failed: %s\n", err.c_str());
    return 1;
  }
  if (argc > 3 && std::string(argv[3]) == "--io-only") {  // I/O surface check, no GPU involved
    const double z[3] = {0, 0, 0};
    const bool ascii = argc > 4 && std::string(argv[4]) == "ascii";
    return bs::ply::write(cloud, 1.0, z, out, ascii, &err) ? 0 : 1;
  }
  const size_t n = cloud.getPointCount();
  std::string raster_prefix;  // --raster=<prefix>: the 2-D branch the reference's main keeps commented out (TMC3.cpp:223-225)
  std::string obj_path;  // --footprints=<file.obj>: extracted_contour (TMC3.cpp:226) on the raster
  std::string bld_path;  // --buildings=<file.obj>: footprints joined with the points and the planes, LoD1 model in mm
  for (int a = 3; a < argc; a++) {
    if (std::string(argv[a]).rfind("--buildings=", 0) == 0)
      bld_path = after_equals(argv[a]);
    if (std::string(argv[a]).rfind("--raster=", 0) == 0)
      raster_prefix = after_equals(argv[a]);
    if (std::string(argv[a]).rfind("--footprints=", 0) == 0)
      obj_path = after_equals(argv[a]);
  }
  try {
    bs::buildingSeg_t<Cloud> seg(cloud);  // bounding box + shift to the origin (TMC3.cpp:209)
    std::vector<VecD> normal;
    std::vector<std::vector<int>> neigh;
    bs::get_Normal_and_K_neighbor<15>(cloud, normal, neigh);
    bs::seg_plane_t<Cloud, VecD, VecI, VecC> h(cloud, normal, neigh, 15);
    auto planes = h.get_planes();
    // The reference never seeds rand() (my_function.cpp:269), i.e. it draws from
    // glibc's seed-1 stream; the HIP runtime consumes rand() values during
    // initialisation, so restore that stream before drawing the colours.
    srand(1);
    h.set_plane_color(planes);
    fprintf(stderr, "tmc3: %zu points, %zu planes\n", n, planes.size());
    if (!raster_prefix.empty() || !obj_path.empty() || !bld_path.empty()) {
      seg.compute_gird_picture();
      if (!raster_prefix.empty())
        seg.save_image(raster_prefix);
      fprintf(stderr, "tmc3: raster %d x %d, ground threshold %.0f mm\n", seg.width, seg.height, seg.ground_th);
    }
    if (!obj_path.empty()) {
      bs_contours c = seg.extracted_contour(obj_path);
      int kept = 0;  // the reference's overlay filter, my_function.cpp:40
      for (int32_t i = 0; i < c.n_contours; i++)
        kept += c.area[i] > 500 && c.perimeter[i] > 100;
      fprintf(stderr, "tmc3: %d footprint contours (%d with area > 500 and perimeter > 100) -> %s\n", c.n_contours,
              kept, obj_path.c_str());
      bs_contours_free(&c);
    }
    if (!bld_path.empty()) {
      bs::building_model m;
      const int32_t np = (int32_t)planes.size();
      seg.extracted_buildings(bld_path, reinterpret_cast<const int32_t*>(cloud.planeIdx.data()), np, m);
      int kept = 0, won = 0;
      long long inside = 0;
      for (int32_t i = 0; i < m.contours.n_contours; i++)
        kept += m.contours.area[i] > 500 && m.contours.perimeter[i] > 100 && m.buildings.n_above[i] > 0;
      for (int32_t p = 0; p < np; p++)
        won += m.plane_building[p] >= 0;
      for (int32_t b : m.building_idx)
        inside += b >= 0;
      fprintf(stderr, "tmc3: %d buildings (%d kept), %lld of %zu points inside one, %d planes, %d with a building -> %s\n",
              m.buildings.n_buildings, kept, inside, n, np, won, bld_path.c_str());
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "tmc3: %s\n", e.what());
    return 1;
  }
  const double zero[3] = {0, 0, 0};
  if (!bs::ply::write(cloud, 1.0, zero, out, false, &err)) {
    fprintf(stderr, "ply write failed: %s\n", err.c_str());
    return 1;
  }
  return 0;
}
