// Runs the scenes of tests/knots_cases.py through the reference's own NonUniformBspline (bspline/src/non_uniform_bspline.cpp,
// compiled unmodified beside this file) on GIVEN knots: the constructor, setKnot -- what traj_server does with the knots
// of Bspline.msg (plan_manage/src/traj_server.cpp:230) -- then getTimeSum and evaluateDeBoorT of the spline and of
// getDerivative applied one, two and three times at the scene's times.  Hex floats in and out.
// in:  n_scenes, then per scene: p n n_t / ctrl [n][3] / knots [n + p + 1] / t [n_t]
// out: per scene one line: getTimeSum, then per time the four points [4][3]
#include <cstdio>
#include <cstdlib>

#include "bspline/non_uniform_bspline.h"

using fast_planner::NonUniformBspline;

static double rd(FILE* f) {
  char tok[64];
  if (fscanf(f, "%63s", tok) != 1) exit(2);
  return strtod(tok, nullptr);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "r");
  FILE* o = fopen(argv[2], "w");
  if (!f || !o) return 2;
  int n_scenes;
  if (fscanf(f, "%d", &n_scenes) != 1) return 2;
  for (int s = 0; s < n_scenes; ++s) {
    int p, n, n_t;
    if (fscanf(f, "%d %d %d", &p, &n, &n_t) != 3) return 2;
    Eigen::MatrixXd ctrl(n, 3);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < 3; ++j) ctrl(i, j) = rd(f);
    Eigen::VectorXd knot(n + p + 1);
    for (int i = 0; i < n + p + 1; ++i) knot(i) = rd(f);
    NonUniformBspline pos(ctrl, p, 1.0);
    pos.setKnot(knot);
    NonUniformBspline vel = pos.getDerivative();
    NonUniformBspline acc = vel.getDerivative();
    NonUniformBspline jerk = acc.getDerivative();
    fprintf(o, "%a", pos.getTimeSum());
    for (int k = 0; k < n_t; ++k) {
      const double t = rd(f);
      for (NonUniformBspline* sp : {&pos, &vel, &acc, &jerk}) {
        const Eigen::VectorXd v = sp->evaluateDeBoorT(t);
        for (int j = 0; j < 3; ++j) fprintf(o, " %a", v(j));
      }
    }
    fprintf(o, "\n");
  }
  fclose(f);
  fclose(o);
  return 0;
}
