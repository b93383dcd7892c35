// solve_tsp_lkh.cpp -- libfuelmi_lkh.so: solveTSPLKH with the reference's signature
// (fuel_planner/utils/lkh_tsp_solver/src/lkh_interface.cpp) over the device ATSP solver of libfuelmi.so, so that
// FastExplorationManager::findGlobalTour (exploration_manager/src/fast_exploration_manager.cpp:327-420) runs unchanged
// when this library is linked in place of the lkh_tsp_solver package.
//
// Parameter file: LKH's "KEY = value" lines (keys without regard to case, '#' lines skipped, the delimiters of
// ReadParameters.c).  Used: PROBLEM_FILE, OUTPUT_TOUR_FILE, TOUR_FILE.  Every other key -- RUNS, MAX_TRIALS,
// MAX_CANDIDATES, SEED, TRACE_LEVEL, GAIN23, ... the controls of LKH's own search -- is ignored: the solve follows
// include/fuelmi.h with the FUELMI_TSP_DEFAULT_* settings.  A '$' in a tour file name is not replaced by the cost.
// Problem file: the TSPLIB header findGlobalTour writes (NAME, TYPE : ATSP, DIMENSION, EDGE_WEIGHT_TYPE : EXPLICIT,
// EDGE_WEIGHT_FORMAT : FULL_MATRIX, COMMENT lines allowed), EDGE_WEIGHT_SECTION, DIMENSION^2 integers, EOF.  Anything
// else is refused.
// Tour file: LKH's (WriteTour.c:33-53): NAME, COMMENT lines, TYPE : TOUR, DIMENSION, TOUR_SECTION, the 1-based ids
// from node 1 on, -1, EOF.
// Failure: a message on stderr and a nonzero return, the tour files removed first.
// Device: the one of the SDFMap the process initialised last through libfuelmi_facade.so, else 0.
#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "fuelmi.h"
#include "lkh_tsp_solver/lkh_interface.h"

// defined by libfuelmi_facade.so when the process has it
extern "C" int fuelmi_facade_last_map_device(void) __attribute__((weak));

namespace {

const char kDelims[] = "= \n\t\r\f\v\xef\xbb\xbf";  // ReadParameters.c:389

std::string upper(std::string s) {
  for (char& ch : s) ch = (char)std::toupper((unsigned char)ch);
  return s;
}

std::string trim(const std::string& s) {
  size_t a = 0, b = s.size();
  while (a < b && std::isspace((unsigned char)s[a])) ++a;
  while (b > a && std::isspace((unsigned char)s[b - 1])) --b;
  return s.substr(a, b - a);
}

bool read_file(const std::string& path, std::string& out) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  char buf[65536];
  size_t n;
  out.clear();
  while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) out.append(buf, n);
  std::fclose(f);
  return true;
}

std::string last_error() {
  const char* e = fuelmi_last_error();
  return e ? e : "?";
}

int fail(const char* fmt, const std::string& a, const std::string& b = "") {
  std::fprintf(stderr, "[fuelmi lkh] solveTSPLKH: ");
  std::fprintf(stderr, fmt, a.c_str(), b.c_str());
  std::fprintf(stderr, "\n");
  return 1;
}

// the TSPLIB problem findGlobalTour writes; "" on success, else what is wrong
std::string parse_problem(const std::string& text, std::string& name, int& dim, std::vector<int32_t>& c) {
  size_t pos = 0;
  bool type = false, ewt = false, ewf = false;
  dim = -1;
  for (;;) {
    if (pos >= text.size()) return "no EDGE_WEIGHT_SECTION";
    size_t eol = text.find('\n', pos);
    if (eol == std::string::npos) eol = text.size();
    const std::string line = trim(text.substr(pos, eol - pos));
    pos = eol + 1;
    if (line.empty()) continue;
    if (upper(line) == "EDGE_WEIGHT_SECTION") break;
    const size_t colon = line.find(':');
    if (colon == std::string::npos) return "header line without ':': " + line;
    const std::string key = upper(trim(line.substr(0, colon))), val = trim(line.substr(colon + 1));
    if (key == "NAME") {
      name = val;
    } else if (key == "COMMENT") {
    } else if (key == "TYPE") {
      if (upper(val) != "ATSP") return "TYPE " + val + " (ATSP only)";
      type = true;
    } else if (key == "DIMENSION") {
      char* end = nullptr;
      const long v = std::strtol(val.c_str(), &end, 10);
      if (val.empty() || *end || v < 1) return "DIMENSION " + val;
      if (v > FUELMI_TSP_MAX_DIM) return "DIMENSION " + val + " above FUELMI_TSP_MAX_DIM";
      dim = (int)v;
    } else if (key == "EDGE_WEIGHT_TYPE") {
      if (upper(val) != "EXPLICIT") return "EDGE_WEIGHT_TYPE " + val + " (EXPLICIT only)";
      ewt = true;
    } else if (key == "EDGE_WEIGHT_FORMAT") {
      if (upper(val) != "FULL_MATRIX") return "EDGE_WEIGHT_FORMAT " + val + " (FULL_MATRIX only)";
      ewf = true;
    } else {
      return "unsupported header key " + key;
    }
  }
  if (!type || !ewt || !ewf || dim < 1) return "TYPE, DIMENSION, EDGE_WEIGHT_TYPE and EDGE_WEIGHT_FORMAT are needed";
  c.assign((size_t)dim * dim, 0);
  const char* p = text.c_str() + std::min(pos, text.size());
  for (size_t k = 0; k < c.size(); ++k) {
    while (*p && std::isspace((unsigned char)*p)) ++p;
    char* end = nullptr;
    errno = 0;
    const long long v = std::strtoll(p, &end, 10);
    if (end == p || errno || v < INT32_MIN || v > INT32_MAX || (*end && !std::isspace((unsigned char)*end)))
      return "entry " + std::to_string(k) + " of EDGE_WEIGHT_SECTION is not a 32-bit integer";
    c[k] = (int32_t)v;
    p = end;
  }
  while (*p && std::isspace((unsigned char)*p)) ++p;
  if (std::strncmp(p, "EOF", 3) != 0) return "more than DIMENSION^2 entries, or no EOF";
  p += 3;
  while (*p && std::isspace((unsigned char)*p)) ++p;
  if (*p) return "text after EOF";
  return "";
}

std::mutex g_mu;
std::map<int, fuelmi_tsp*> g_solvers;  // one per device, for the life of the process

}  // namespace

int solveTSPLKH(const char* input_file) {
  if (!input_file) return fail("%s", "no parameter file");
  std::string par;
  if (!read_file(input_file, par)) return fail("cannot read the parameter file %s", input_file);
  std::string prob_file, tour_files[2];  // OUTPUT_TOUR_FILE, TOUR_FILE
  std::vector<char> buf(par.begin(), par.end());
  buf.push_back('\0');
  char* s1 = nullptr;
  for (char* line = strtok_r(buf.data(), "\n", &s1); line; line = strtok_r(nullptr, "\n", &s1)) {
    char* s2 = nullptr;
    char* kw = strtok_r(line, kDelims, &s2);
    if (!kw || kw[0] == '#') continue;
    const std::string key = upper(kw);
    char* val = strtok_r(nullptr, kDelims, &s2);
    if (key == "PROBLEM_FILE" && val) prob_file = val;
    else if (key == "OUTPUT_TOUR_FILE" && val) tour_files[0] = val;
    else if (key == "TOUR_FILE" && val) tour_files[1] = val;
  }
  // no tour of an earlier call may survive a failure of this one
  for (const std::string& f : tour_files)
    if (!f.empty()) std::remove(f.c_str());
  if (prob_file.empty()) return fail("%s names no PROBLEM_FILE", input_file);
  std::string text, name = "single";
  if (!read_file(prob_file, text)) return fail("cannot read the problem file %s", prob_file);
  int dim = 0;
  std::vector<int32_t> c;
  const std::string why = parse_problem(text, name, dim, c);
  if (!why.empty()) return fail("problem file %s refused: %s", prob_file, why);
  int device = fuelmi_facade_last_map_device ? fuelmi_facade_last_map_device() : -1;
  if (device < 0) device = 0;
  std::vector<int> order(dim);
  int64_t cost = 0;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    fuelmi_tsp*& t = g_solvers[device];
    if (!t) {
      fuelmi_init(0);
      const fuelmi_tsp_cfg cfg = {FUELMI_TSP_DEFAULT_RESTARTS, FUELMI_TSP_DEFAULT_KICKS, FUELMI_TSP_DEFAULT_EXACT_MAX, 0};
      if (fuelmi_tsp_create(device, &cfg, &t) != FUELMI_OK) {
        t = nullptr;
        return fail("fuelmi_tsp_create: %s", last_error());
      }
    }
    const int dim_ptr[2] = {0, dim};
    int method = 0;
    if (fuelmi_tsp_solve(t, 1, dim_ptr, c.data(), order.data(), &cost, &method) != FUELMI_OK)
      return fail("fuelmi_tsp_solve: %s", last_error());
  }
  for (const std::string& f : tour_files) {
    if (f.empty()) continue;
    FILE* out = std::fopen(f.c_str(), "w");
    if (!out) return fail("cannot write the tour file %s", f);
    std::fprintf(out, "NAME : %s.%lld.tour\n", name.c_str(), (long long)cost);
    std::fprintf(out, "COMMENT : Length = %lld\n", (long long)cost);
    std::fprintf(out, "COMMENT : Found by the fuelmi device ATSP solver\n");
    std::fprintf(out, "TYPE : TOUR\nDIMENSION : %d\nTOUR_SECTION\n", dim);
    for (int k = 0; k < dim; ++k) std::fprintf(out, "%d\n", order[k] + 1);
    std::fprintf(out, "-1\nEOF\n");
    if (std::fclose(out) != 0) {
      std::remove(f.c_str());
      return fail("writing the tour file %s failed", f);
    }
  }
  return 0;
}
