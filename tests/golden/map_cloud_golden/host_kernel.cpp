// A host build of the three cloud kernels' own text (fuel_amd/csrc/map_cloud.hip from "namespace {" to the host code, cut
// out by tests/golden/check_map_cloud_host_build.py into kernel.inc) on the lanes of tests/golden/host_lanes.h.  Every
// device array is a heap block of its exact size -- the workgroup words [nwg], the total, the pinned word, the points
// [min(cap, voxels)][3] -- and a plane is the W words that cover the map followed by exactly ONE word of its zero
// margin, the one a chunk that ends in the plane's last word may load; a read past it is reported.
//   host_kernel <planes.bin> <scenes.txt> <out.bin>
#include "host_lanes.h"
#include "kernel.inc"
}  // namespace (kernel.inc leaves it open)

struct State {
  Geo g;
  std::unique_ptr<u64[]> plane[3];  // occupied, unknown, inflated: W + 1 words each
};

int main(int argc, char** argv) {
  if (argc < 4) return 1;
  std::ifstream pin(argv[1], std::ios::binary);
  int n_states = 0;
  pin.read(reinterpret_cast<char*>(&n_states), 4);
  std::vector<State> states(n_states);
  for (State& s : states) {
    int nv[3];
    double gd[4];
    pin.read(reinterpret_cast<char*>(nv), 12);
    pin.read(reinterpret_cast<char*>(gd), 32);
    Geo& g = s.g;
    memset(&g, 0, sizeof(g));
    g.nx = nv[0], g.ny = nv[1], g.nz = nv[2];
    g.nyz = g.ny * g.nz, g.N = g.nx * g.nyz, g.W = (g.N + 63) / 64;
    g.res = gd[0], g.res_inv = 1 / gd[0];
    g.org[0] = gd[1], g.org[1] = gd[2], g.org[2] = gd[3];
    for (auto& p : s.plane) {
      p.reset(new u64[g.W + 1]);
      pin.read(reinterpret_cast<char*>(p.get()), (size_t)g.W * 8);
      p[g.W] = 0ull;
    }
  }
  if (!pin) return 2;
  std::ifstream in(argv[2]);
  FILE* out = fopen(argv[3], "wb");
  int n_scenes = 0;
  in >> n_scenes;
  for (int i = 0; i < n_scenes; ++i) {
    int si, kind, lo[3], hi[3];
    long cap;
    std::string a, b;
    in >> si >> kind >> lo[0] >> lo[1] >> lo[2] >> hi[0] >> hi[1] >> hi[2] >> a >> b >> cap;
    const State& s = states[si];
    CloudArgs C;
    memset(&C, 0, sizeof(C));
    C.plane = s.plane[kind == 0 ? 0 : kind == 3 ? 2 : 1].get();
    C.invert = kind == 2;
    for (int k = 0; k < 3; ++k) C.lo[k] = lo[k];
    const long xlen = hi[0] - lo[0] + 1;
    C.ylen = hi[1] - lo[1] + 1, C.zlen = hi[2] - lo[2] + 1;
    C.cpl = (C.zlen + 63) / 64;
    C.n_items = (int)(xlen * C.ylen * C.cpl);
    C.nwg = (C.n_items + CL_WG - 1) / CL_WG;
    C.z_low = strtod(a.c_str(), nullptr), C.z_high = strtod(b.c_str(), nullptr);
    const long voxels = xlen * C.ylen * C.zlen;
    const long n_out = std::min(cap, voxels);
    std::unique_ptr<u32[]> wg(new u32[C.nwg]);
    std::unique_ptr<u32> total(new u32), total_pin(new u32);
    std::unique_ptr<float[]> pts(new float[(size_t)n_out * 3]);
    for (int k = 0; k < C.nwg; ++k) wg[k] = 0xDEADBEEFu;  // stale words of a grown scratch
    for (long k = 0; k < n_out * 3; ++k) memcpy(&pts[k], "\xA5\xA5\xA5\xA5", 4);
    *total = *total_pin = 0x7FFFFFFFu;
    C.wg = wg.get(), C.total = total.get(), C.total_pin = total_pin.get(), C.out = pts.get(), C.cap = (u32)n_out;
    launch(C.nwg, CL_WG, 0, [&] { k_cloud_count(s.g, C); });
    launch(1, CL_SCAN, 0, [&] { k_cloud_scan(C); });
    if (n_out) launch(C.nwg, CL_WG, 0, [&] { k_cloud_write(s.g, C); });
    if (*total != *total_pin) return 3;
    const int tot = (int)*total, nw = (int)n_out;
    fwrite(&tot, 4, 1, out);
    fwrite(&nw, 4, 1, out);
    fwrite(pts.get(), 12, (size_t)n_out, out);  // the whole buffer: the tail behind the points must still be the fill
  }
  fclose(out);
  return 0;
}
