// A host build of the inflation kernels' own text -- k_box_and, k_inflate_yz, k_inflate_x, k_inflate_fused and the launch
// ranges (fuel_amd/csrc/map_core.hip), box_mask_word and bit_range (fuelmi_internal.h), cut out by
// tests/golden/check_inflate_host_build.py into kernel.inc -- on the lanes of tests/golden/host_lanes.h.  Every bit-plane
// is a heap block of exactly W + 2 * margin_words + 2 words, as plane_alloc makes it; the fused kernel's LDS is a block of
// exactly lds_f bytes between guard zones.  A job is one map with a sequence of calls: the two scratch planes live as
// long as the job and START FILLED with a pattern (all but their last two words, which no kernel ever writes), as the
// stale words of an earlier, larger call would be: a word that is read without having been written in the same call shows
// as a differing bit.  The launches are fuelmi_map_inflate_local's, from the plan it runs.
//   host_kernel <jobs.bin> <out.bin>
// jobs.bin: int n_jobs; per job: int nx, ny, nz, step, n_calls; u64 occupied[W]; u64 inflated[W]; per call: int lo[3],
// hi[3], pin.  out.bin: per call: int kernel that ran; u64 inflated[W].
#include "host_lanes.h"
static Idx gridDim_;  // (k_inflate_x deals eighths of its grid to the XCDs)
#define gridDim gridDim_
#include "kernel.inc"

struct HostPlane {
  std::unique_ptr<u64[]> base;
  u64* p = nullptr;
  HostPlane(const Geo& g, int margin, u64 fill) {
    const size_t words = (size_t)g.W + 2 * (size_t)margin + 2;  // plane_alloc's
    base.reset(new u64[words]);
    for (size_t i = 0; i < words; ++i) base[i] = i + 2 < words ? fill : 0ull;
    p = base.get() + margin;
  }
};

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  std::ifstream in(argv[1], std::ios::binary);
  FILE* out = fopen(argv[2], "wb");
  auto geti = [&] {
    int v = 0;
    in.read(reinterpret_cast<char*>(&v), 4);
    return v;
  };
  const int n_jobs = geti();
  for (int j = 0; j < n_jobs; ++j) {
    Geo g;
    memset(&g, 0, sizeof(g));
    g.nx = geti(), g.ny = geti(), g.nz = geti();
    const int step = geti(), n_calls = geti();
    g.nyz = g.ny * g.nz, g.N = g.nx * g.nyz, g.W = (g.N + 63) / 64;
    const int margin = inflate_margin_words(g, step);
    HostPlane occ(g, margin, 0ull), infl(g, margin, 0ull), tmp(g, margin, 0xA5A5A5A5A5A5A5A5ull),
        tmp2(g, margin, 0x5A5A5A5A5A5A5A5Aull);
    in.read(reinterpret_cast<char*>(occ.p), (size_t)g.W * 8);
    in.read(reinterpret_cast<char*>(infl.p), (size_t)g.W * 8);
    for (int c = 0; c < n_calls; ++c) {
      Box3 b;
      for (int k = 0; k < 3; ++k) b.lo[k] = geti();
      for (int k = 0; k < 3; ++k) b.hi[k] = geti();
      const int pin = geti();
      if (!in) return 2;
      const InflatePlan P = inflate_plan(g, step, b, pin);
      if (P.margin_words != margin) return 3;
      int rc = 0;
      if (P.kernel == FUELMI_INFLATE_FUSED) {
        if (P.whole)
          rc = launch(P.grid_fused, 256, P.lds_f, [&] { k_inflate_fused<2, true>(g, b, occ.p, infl.p, P.out_lo, P.out_hi, margin); });
        else
          rc = launch(P.grid_fused, 256, P.lds_f, [&] { k_inflate_fused<2, false>(g, b, occ.p, infl.p, P.out_lo, P.out_hi, margin); });
      } else {
        const u64* S = P.whole ? occ.p : tmp.p;
        if (!P.whole) rc = launch(P.grid_box, 256, 0, [&] { k_box_and(g, b, occ.p, tmp.p, P.s_lo, P.s_hi); });
        if (!rc && step == 2) rc = launch(P.grid_yz, 256, 0, [&] { k_inflate_yz<2>(g, step, S, tmp2.p, P.t_lo, P.t_hi); });
        if (!rc && step != 2) rc = launch(P.grid_yz, 256, 0, [&] { k_inflate_yz<0>(g, step, S, tmp2.p, P.t_lo, P.t_hi); });
        gridDim_.x = P.grid_x;
        if (!rc) rc = launch(P.grid_x, 256, 0, [&] { k_inflate_x(g, b, step, tmp2.p, infl.p, P.out_lo, P.out_hi); });
      }
      if (rc) return rc;
      // the margins of the two state planes stay zero whatever runs
      for (int k = 1; k <= margin; ++k)
        if (occ.p[-k] | infl.p[-k] | occ.p[g.W - 1 + k] | infl.p[g.W - 1 + k]) return 4;
      fwrite(&P.kernel, 4, 1, out);
      fwrite(infl.p, 8, (size_t)g.W, out);
    }
  }
  fclose(out);
  return 0;
}
