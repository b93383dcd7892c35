// A host build of k_info_gain's and k_yaw_path's own text and of the host's view setup (fuel_amd/csrc/info_gain.hip between
// "namespace {" and the argument checks, cut out by tests/golden/check_heading_host_build.py into kernel.inc) on the lanes
// of tests/golden/host_lanes.h.  The bit planes, the groups, the views, the control points and the result arrays are heap
// blocks of their exact size.  Reads the launches check_heading_host_build.py writes and prints one line per group or
// problem: the integers, then the bits of the doubles.
//   host_kernel <in.txt>
// in.txt: the maps (nx ny nz, origin, res_inv, res, box in metres, box in indices, the files of the unknown and occupied
// planes as 64-bit words), then launches
//   G map n <gain cfg>, per group: pos, n_yaw, yaws, path; then n_path, per path n_ctrl <points>
//   P map n h max_layer yaw_diff max_yaw_rate w given <gain cfg>, per problem: n_layer dt <pts> <yaws>, n_ctrl <points>,
//     and with given = 1 the gains [max_layer][2h + 1]
#include "host_lanes.h"
#include "kernel.inc"
}  // namespace (kernel.inc leaves it open)

struct HostMap {
  Geo g;
  double bmind[3], bmaxd[3];
  int bmin[3], bmax[3];
  std::vector<u64> unk, occ;
};

static void read_cfg(std::ifstream& in, fuelmi_gain_cfg& c) {
  in >> c.weight_type >> c.in_box >> c.factor >> c.max_yaw >> c.max_ctrl;
  c.far = num(in), c.top_ang = num(in), c.left_ang = num(in), c.right_ang = num(in), c.lambda1 = num(in), c.lambda2 = num(in);
}

// the gain kernel over the groups; false: a guard zone was hit
static bool run_gain(const HostMap& M, const fuelmi_gain_cfg& c, std::vector<GainGroup>& groups, std::vector<GainView>& views,
                     const std::vector<int>& nc, const std::vector<double>& ctrl, std::vector<double>& gain,
                     std::vector<int>& n_cand, std::vector<int>& n_vis, std::vector<int>& n_rays) {
  GainArgs A;
  memset(&A, 0, sizeof(A));
  A.cfg = c, A.n_group = (int)groups.size();
  int cells = 0;
  for (const GainGroup& G : groups) cells = std::max(cells, G.n_yaw > 0 ? G.cells : 0);
  if (cells == 0) return true;
  A.lds_cells = (cells + 63) & ~63;
  for (int k = 0; k < 3; ++k) A.off[k] = 0.5 - M.g.org[k] / M.g.res, A.bmin[k] = M.bmin[k], A.bmax[k] = M.bmax[k];
  A.unk = M.unk.data(), A.occ = M.occ.data();
  A.groups = groups.data(), A.views = views.data(), A.n_ctrl = nc.data(), A.ctrl = ctrl.data();
  A.gain = gain.data(), A.n_cand = n_cand.data(), A.n_visible = n_vis.data(), A.n_rays = n_rays.data();
  const bool weighted = c.weight_type == FUELMI_GAIN_NON_UNIFORM;
  return launch(A.n_group, IG_NT, ig_lds(A.lds_cells, weighted, c.max_ctrl), [&] { k_info_gain(M.g, A); }) == 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  std::ifstream in(argv[1]);
  int n_maps;
  in >> n_maps;
  std::vector<HostMap> maps(n_maps);
  for (HostMap& M : maps) {
    Geo& g = M.g;
    memset(&g, 0, sizeof(g));
    in >> g.nx >> g.ny >> g.nz;
    for (double& o : g.org) o = num(in);
    g.res_inv = num(in), g.res = num(in);
    for (double& v : M.bmind) v = num(in);
    for (double& v : M.bmaxd) v = num(in);
    in >> M.bmin[0] >> M.bmin[1] >> M.bmin[2] >> M.bmax[0] >> M.bmax[1] >> M.bmax[2];
    g.nyz = g.ny * g.nz, g.N = g.nx * g.nyz, g.W = (g.N + 63) / 64;
    std::string pu, po;
    in >> pu >> po;
    M.unk.resize(g.W), M.occ.resize(g.W);  // exactly the map's words: the sanitizer sees a read past them
    std::ifstream(pu, std::ios::binary).read(reinterpret_cast<char*>(M.unk.data()), g.W * sizeof(u64));
    std::ifstream(po, std::ios::binary).read(reinterpret_cast<char*>(M.occ.data()), g.W * sizeof(u64));
  }
  std::string kind;
  while (in >> kind) {
    int map, n;
    in >> map >> n;
    const HostMap& M = maps[map];
    if (kind == "G") {
      fuelmi_gain_cfg c;
      read_cfg(in, c);
      const size_t my = c.max_yaw;
      std::vector<GainGroup> groups(n);
      std::vector<GainView> views(n * my);
      memset(groups.data(), 0, n * sizeof(GainGroup)), memset(views.data(), 0, views.size() * sizeof(GainView));
      std::vector<int> status(n, 0);
      for (int b = 0; b < n; ++b) {
        GainGroup& G = groups[b];
        for (double& v : G.pos) v = num(in);
        in >> G.n_yaw;
        for (int v = 0; v < G.n_yaw; ++v) gain_view_setup(c, M.g, M.bmind, M.bmaxd, G.pos, num(in), views[b * my + v]);
        in >> G.path;
        if (!gain_group_box(c, views.data() + b * my, G)) G.n_yaw = 0, status[b] = -1;
      }
      int n_path;
      in >> n_path;
      std::vector<int> nc(n_path);
      std::vector<double> ctrl((size_t)n_path * c.max_ctrl * 3, 1e300);  // (a read past a path's own points shows)
      for (int p = 0; p < n_path; ++p) {
        in >> nc[p];
        for (int k = 0; k < 3 * nc[p]; ++k) ctrl[(size_t)p * c.max_ctrl * 3 + k] = num(in);
      }
      std::vector<double> gain(n * my, 0.0);
      std::vector<int> n_cand(n * my, 0), n_vis(n * my, 0), n_rays(n, 0);
      if (!run_gain(M, c, groups, views, nc, ctrl, gain, n_cand, n_vis, n_rays)) return 9;
      for (int b = 0; b < n; ++b) {
        std::printf("%d %d", status[b], n_rays[b]);
        for (size_t v = 0; v < my; ++v) std::printf(" %d %d %016llx", n_cand[b * my + v], n_vis[b * my + v], bits(gain[b * my + v]));
        std::printf("\n");
      }
    } else {
      fuelmi_yawpath_cfg Y;
      int given;
      in >> Y.half_vert_num >> Y.max_layer;
      Y.yaw_diff = num(in), Y.max_yaw_rate = num(in), Y.w = num(in);
      in >> given;
      read_cfg(in, Y.gain);
      fuelmi_gain_cfg c = Y.gain;
      c.max_yaw = 2 * Y.half_vert_num + 1;
      const size_t ml = Y.max_layer, nv = c.max_yaw, ng = n * ml;
      std::vector<int> n_layer(n), over(n, 0), nc(n, 0);
      std::vector<double> dt(n), pts(ng * 3, 1e300), yaws(ng, 1e300), ctrl((size_t)n * c.max_ctrl * 3, 1e300), gains(ng * nv, 0.0);
      std::vector<GainGroup> groups(ng);
      std::vector<GainView> views(ng * nv);
      memset(groups.data(), 0, ng * sizeof(GainGroup)), memset(views.data(), 0, views.size() * sizeof(GainView));
      for (int b = 0; b < n; ++b) {
        in >> n_layer[b];
        dt[b] = num(in);
        for (int k = 0; k < 3 * n_layer[b]; ++k) pts[b * ml * 3 + k] = num(in);
        for (int k = 0; k < n_layer[b]; ++k) yaws[b * ml + k] = num(in);
        in >> nc[b];
        for (int k = 0; k < 3 * nc[b]; ++k) ctrl[(size_t)b * c.max_ctrl * 3 + k] = num(in);
        if (given)
          for (size_t k = 0; k < ml * nv; ++k) gains[b * ml * nv + k] = num(in);
        for (int i = 1; !given && i < n_layer[b] - 1; ++i) {  // as fuelmi_map_yaw_paths lays the groups out
          const size_t gi = b * ml + i;
          GainGroup& G = groups[gi];
          for (int k = 0; k < 3; ++k) G.pos[k] = pts[gi * 3 + k];
          G.n_yaw = (int)nv, G.path = b;
          for (int j = 0; j < (int)nv; ++j)
            gain_view_setup(c, M.g, M.bmind, M.bmaxd, G.pos, yaws[gi] + double(j - Y.half_vert_num) * Y.yaw_diff, views[gi * nv + j]);
          if (!gain_group_box(c, views.data() + gi * nv, G)) G.n_yaw = 0, over[b] = 1;
        }
      }
      std::vector<int> n_cand(ng * nv, 0), n_vis(ng * nv, 0), n_rays(ng, 0);
      if (!given && !run_gain(M, c, groups, views, nc, ctrl, gains, n_cand, n_vis, n_rays)) return 9;
      std::vector<int> status(n, 7), pv(ng, 0);
      std::vector<double> path(ng, 0.0), gv(ng * nv, 0.0);
      YawPathArgs A;
      memset(&A, 0, sizeof(A));
      A.n_prob = n, A.max_layer = Y.max_layer, A.nv = (int)nv, A.h = Y.half_vert_num;
      A.yaw_diff = Y.yaw_diff, A.max_yaw_rate = Y.max_yaw_rate, A.w = Y.w;
      A.n_layer = n_layer.data(), A.yaws = yaws.data(), A.dt = dt.data(), A.gains = gains.data(), A.over = over.data();
      A.status = status.data(), A.path = path.data(), A.path_vertex = pv.data(), A.g_value = gv.data();
      if (launch(n, YP_NT, 0, [&] { k_yaw_path(A); })) return 9;
      for (int b = 0; b < n; ++b) {
        std::printf("%d", status[b]);
        for (int i = 0; i < n_layer[b]; ++i) std::printf(" %d %d %016llx", n_rays[b * ml + i], pv[b * ml + i], bits(path[b * ml + i]));
        for (int i = 0; i < n_layer[b]; ++i)
          for (size_t j = 0; j < nv; ++j)
            std::printf(" %016llx %016llx", bits(gains[(b * ml + i) * nv + j]), bits(gv[(b * ml + i) * nv + j]));
        std::printf("\n");
      }
    }
  }
  return 0;
}
