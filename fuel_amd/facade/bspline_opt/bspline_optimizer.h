// bspline_opt/bspline_optimizer.h -- drop-in for the reference header of the same name
// (fuel_planner/bspline_opt/include/bspline_opt/bspline_optimizer.h:18-141).
//
// What is behind the same API here: combineCost and every calc*Cost term are one HIP kernel against the
// device ESDF; optimize() is one kernel launch that runs the whole solve (start clamping, bounds,
// best-variable tracking, evaluation cap and xtol_rel as the reference configures NLopt; the iteration
// is a box-projected L-BFGS because NLopt is a third-party library that is absent here -- final costs
// are comparable with NLopt's, iterates are not).
#ifndef _BSPLINE_OPTIMIZER_H_
#define _BSPLINE_OPTIMIZER_H_

#include <Eigen/Eigen>

#include <memory>
#include <vector>

#include <ros/ros.h>

// struct ViewConstraint comes from the visibility module, as in the reference header (:5); in this
// repository's own build the stand-in under facade/standin/ supplies it
#include <active_perception/traj_visibility.h>

#include "fuelmi.h"

using std::shared_ptr;
using std::unique_ptr;
using std::vector;

namespace fast_planner {
class EDTEnvironment;

class BsplineOptimizer {
public:
  typedef unique_ptr<BsplineOptimizer> Ptr;

  // bit masks of the cost terms and the two usual combinations (values: bspline_optimizer.cpp:10-23)
  static const int SMOOTHNESS, DISTANCE, FEASIBILITY, START, END, GUIDE, WAYPOINTS, VIEWCONS, MINTIME;
  static const int GUIDE_PHASE, NORMAL_PHASE;

  BsplineOptimizer() {}
  ~BsplineOptimizer() {}

  // configuration
  void setParam(ros::NodeHandle& node);
  void setEnvironment(const shared_ptr<EDTEnvironment>& env);

  // per-solve inputs
  void setCostFunction(const int& cost_mask);
  void setBoundaryStates(const vector<Eigen::Vector3d>& start, const vector<Eigen::Vector3d>& end);
  void setTimeLowerBound(const double& lower);
  void setGuidePath(const vector<Eigen::Vector3d>& guide);
  void setWaypoints(const vector<Eigen::Vector3d>& points, const vector<int>& indices);
  void setViewConstraint(const ViewConstraint& constraint);
  void enableDynamic(double time_start);

  // the solve: control points (rows) and knot span in, optimised values out
  void optimize(Eigen::MatrixXd& ctrl_pts, double& knot_span, const int& cost_mask, const int& max_num_id,
                const int& max_time_id);
  void optimize();

  // addition: the body of FastPlannerManager::planExploreTraj from the way-points to the solved spline
  // (plan_manage/src/planner_manager.cpp:270-312) in four device calls: fuelmi_map_waypoint_trajs (segment times,
  // waypointsTraj, getLength, seg_num, samples, boundary derivatives) -> parameterizeToBspline -> getBoundaryStates(2, 0)
  // -> setBoundaryStates, setTimeLowerBound (time_lb > 0) -> optimize(ctrl_pts, dt, cost_mask, 1, 1).
  // Returns FUELMI_WPTRAJ_OK, or without touching ctrl_pts / dt: FUELMI_WPTRAJ_FEW (fewer than three points, the empty
  // tour included), FUELMI_WPTRAJ_DEGENERATE (two consecutive points coincide), or the negative FUELMI_E* of a call
  // that failed.
  int planThroughWaypoints(const vector<Eigen::Vector3d>& tour, const Eigen::Vector3d& cur_vel,
                           const Eigen::Vector3d& cur_acc, double max_vel, double ctrl_pt_dist, int cost_mask,
                           double time_lb, Eigen::MatrixXd& ctrl_pts, double& dt);
  // addition: the body of FastPlannerManager::kinodynamicReplan (plan_manage/src/planner_manager.cpp:124-185) -- the
  // mid-range branch of planExploreMotion -- without the reference's KinodynamicAstar on the host: the search with its
  // retry and getSamples in one device call (fuelmi_map_kino_paths, include/fuelmi.h; `search` holds the search/*
  // parameters, its ts / seg_num / max_* fields are set here: ts = ctrl_pt_dist / max_vel), then parameterizeToBspline,
  // getBoundaryStates(2, 0), setBoundaryStates, setTimeLowerBound when time_lb > 0 and optimize(ctrl_pts, dt, cost_mask,
  // 1, 1).  Returns the search's status (FUELMI_KINO_REACH_HORIZON / _REACH_END / _NEAR_END) with ctrl_pts / dt filled,
  // or without touching them: FUELMI_KINO_NO_PATH, FUELMI_KINO_CLOSE_GOAL (the reference returns false for both), or the
  // negative FUELMI_E* of a call that failed.  init_ctrl_pts_ / init_knot_span_ / final_cost_ as below.
  int planKinodynamic(const Eigen::Vector3d& start_pt, const Eigen::Vector3d& start_vel, const Eigen::Vector3d& start_acc,
                      const Eigen::Vector3d& end_pt, const Eigen::Vector3d& end_vel, const fuelmi_kino_cfg& search,
                      double max_vel, double ctrl_pt_dist, int cost_mask, double time_lb, Eigen::MatrixXd& ctrl_pts,
                      double& dt);
  int kino_iter_num_ = 0, kino_use_node_num_ = 0, kino_which_ = 0;  // diagnostics of the last planKinodynamic
  // diagnostics of the last planThroughWaypoints: what it handed to the solve, and the solve's final cost
  Eigen::MatrixXd init_ctrl_pts_;
  double init_knot_span_ = 0.0, final_cost_ = 0.0;

  // additions: the bodies of FastPlannerManager::planYawExplore (plan_manage/src/planner_manager.cpp:774-853) and
  // ::planYaw (:695-758) in one device call each (fuelmi_map_plan_yaws, include/fuelmi.h): the way-points by look-ahead
  // on the uniform position spline (pos_ctrl rows, degree pos_degree, knot span pos_dt), the unwrap chain, the initial
  // control points and THE MINIMISER of the yaw objective (the reference's NLopt run iterates towards it), with this
  // optimiser's own weights and its environment's map.  yaw_ctrl ((seg_num + 3) x 1) and dt_yaw are what the caller
  // hands to setUniformBspline(yaw, 3 / bspline_degree_, dt_yaw) and getDerivative() twice; planYaw's path_yaw (may be
  // null) receives the way-points (plan_data_.path_yaw_).  Both return the problem's status, and touch the outputs only
  // when it is FUELMI_YAW_OK: FUELMI_YAW_DEGENERATE (start (0, 0, 0) to end 0: the reference divides by pt_dist_ = 0)
  // or the negative FUELMI_E* of a call that failed.
  int planYawExplore(const Eigen::MatrixXd& pos_ctrl, int pos_degree, double pos_dt, const Eigen::Vector3d& start_yaw,
                     double end_yaw, bool lookfwd, double relax_time, Eigen::MatrixXd& yaw_ctrl, double& dt_yaw);
  int planYaw(const Eigen::MatrixXd& pos_ctrl, int pos_degree, double pos_dt, const Eigen::Vector3d& start_yaw,
              Eigen::MatrixXd& yaw_ctrl, double& dt_yaw, std::vector<double>* path_yaw);
  // ... on a position spline whose knots were moved (setKnot): `knots` holds pos_ctrl.rows() + pos_degree + 1 of them,
  // what adjustTime returns (fuelmi_map_plan_yaws_knots).  The yaw spline that comes out is uniform, as ever.
  int planYaw(const Eigen::MatrixXd& pos_ctrl, int pos_degree, const Eigen::VectorXd& knots, const Eigen::Vector3d& start_yaw,
              Eigen::MatrixXd& yaw_ctrl, double& dt_yaw, std::vector<double>* path_yaw);

  // addition: the body of FastPlannerManager::checkTrajCollision (plan_manage/src/planner_manager.cpp:96-118) in one
  // device call (fuelmi_map_check_trajs, include/fuelmi.h) on the uniform position spline (pos_ctrl rows, degree, knot
  // span dt) at time t_now since the trajectory's start, against the inflated plane of this optimiser's environment's
  // map as the device holds it: no host mirror is read, so it answers with the inflate mirror switched off.  Returns
  // the reference's value; `distance` is written only when the result is false, as the reference does.  A call that
  // fails, or a point the reference could not index (FUELMI_TRAJCHK_NONFINITE), is reported as a collision at distance 0.
  bool checkTrajCollision(const Eigen::MatrixXd& pos_ctrl, int degree, double dt, double t_now, double& distance);
  // ... on the knots adjustTime returned (pos_ctrl.rows() + degree + 1 of them; fuelmi_map_check_trajs_knots): what the
  // safety callback walks once local_data_.position_traj_ has been time-adjusted
  bool checkTrajCollision(const Eigen::MatrixXd& pos_ctrl, int degree, const Eigen::VectorXd& knots, double t_now,
                          double& distance);

  // addition: the two things the reference does with a finished trajectory, each in one device call
  // (fuelmi_map_sample_trajs, include/fuelmi.h) on the uniform position spline (pos_ctrl rows, degree, knot span dt) and
  // the uniform yaw spline (yaw_ctrl rows x 1, yaw_degree, yaw_dt; 0 rows: none, the yaw outputs are 0).
  // evaluateCommand is the body of traj_server's cmdCallback (plan_manage/src/traj_server.cpp:266-290, 328-339) for a
  // whole tape of times t since the trajectory's start: t_stop (may be null) is what replanCallback left in
  // traj_duration_; status receives FUELMI_TRAJSMP_IN / _PAST / _INVALID per tick, pos / vel / acc / jerk one row per
  // tick, yaw one row (yaw, yaw rate, yaw acceleration) per tick; flight8 (may be null) is the flight record, carried
  // from call to call.  replanState is the FSM's replan start state at t_r (fast_exploration_fsm.cpp:86-95): start_yaw =
  // (yaw, yaw rate, yaw acceleration).  Both return false, and touch no output, when the call fails.
  bool evaluateCommand(const Eigen::MatrixXd& pos_ctrl, int degree, double dt, const Eigen::MatrixXd& yaw_ctrl,
                       int yaw_degree, double yaw_dt, const std::vector<double>& t, const double* t_stop,
                       std::vector<int>& status, Eigen::MatrixXd& pos, Eigen::MatrixXd& vel, Eigen::MatrixXd& acc,
                       Eigen::MatrixXd& jerk, Eigen::MatrixXd& yaw, double* flight8);
  bool replanState(const Eigen::MatrixXd& pos_ctrl, int degree, double dt, const Eigen::MatrixXd& yaw_ctrl, int yaw_degree,
                   double yaw_dt, double t_r, Eigen::Vector3d& start_pt, Eigen::Vector3d& start_vel,
                   Eigen::Vector3d& start_acc, Eigen::Vector3d& start_yaw);
  // ... with the position spline on the knots adjustTime returned (pos_ctrl.rows() + degree + 1 of them) -- traj_server's
  // pos_traj.setKnot(knots) (traj_server.cpp:230) before it samples -- through fuelmi_map_sample_trajs_knots; the yaw
  // spline stays uniform (Bspline.msg carries only yaw_dt)
  bool evaluateCommand(const Eigen::MatrixXd& pos_ctrl, int degree, const Eigen::VectorXd& knots, const Eigen::MatrixXd& yaw_ctrl,
                       int yaw_degree, double yaw_dt, const std::vector<double>& t, const double* t_stop,
                       std::vector<int>& status, Eigen::MatrixXd& pos, Eigen::MatrixXd& vel, Eigen::MatrixXd& acc,
                       Eigen::MatrixXd& jerk, Eigen::MatrixXd& yaw, double* flight8);
  bool replanState(const Eigen::MatrixXd& pos_ctrl, int degree, const Eigen::VectorXd& knots, const Eigen::MatrixXd& yaw_ctrl,
                   int yaw_degree, double yaw_dt, double t_r, Eigen::Vector3d& start_pt, Eigen::Vector3d& start_vel,
                   Eigen::Vector3d& start_acc, Eigen::Vector3d& start_yaw);

  // addition: the half of NonUniformBspline that moves knots and measures a spline (bspline/src/non_uniform_bspline.cpp
  // :135-176, :267-487), each in one device call (fuelmi_map_adjust_trajs, include/fuelmi.h) on the position spline
  // (pos_ctrl rows, degree) with the knots in `knots`: pos_ctrl.rows() + degree + 1 of them, or an EMPTY vector for the
  // uniform knots of the span dt.  The limits are setPhysicalLimits' (the reference's callers pass max_vel_ / max_acc_,
  // the defaults here) and the constants both reference callers use.
  struct TrajAdjust {
    double limit_vel = 2.0, limit_acc = 2.0, limit_ratio = 1.1, lengthen_cap = 1.01, length_res = 0.01, stat_step = 0.01;
    int realloc_iters = 3;
  };
  // what one spline comes back with: info[FUELMI_TRAJADJ_I_*] and metrics[FUELMI_TRAJADJ_M_*]
  struct TrajMetrics {
    int info[FUELMI_TRAJADJ_NI];
    double metrics[FUELMI_TRAJADJ_NM];
    int status() const { return info[FUELMI_TRAJADJ_I_STATUS]; }
    bool feasible() const { return info[FUELMI_TRAJADJ_I_FEASIBLE_OUT] != 0; }
    double duration() const { return metrics[FUELMI_TRAJADJ_M_DURATION_OUT]; }
    double length() const { return metrics[FUELMI_TRAJADJ_M_LENGTH]; }
    double jerk() const { return metrics[FUELMI_TRAJADJ_M_JERK]; }
  };
  // adjustTime: ops = FUELMI_TRAJADJ_LENGTHEN (lengthenTime(min(cap, ratio_in ? *ratio_in : checkRatio())), the first
  // half of reparamBspline, planner_manager.cpp:534-536) | FUELMI_TRAJADJ_REALLOC (the checkFeasibility /
  // reallocateTime loop, :222-230) | FUELMI_TRAJADJ_RESAMPLE (the points of :541-543 into samples, one row each; their
  // step is metrics[FUELMI_TRAJADJ_M_DT_OUT], what parameterizeToBspline takes next).  knots receives the adjusted
  // knots (setKnot on the reference's class continues from them), samples may be null.  trajectoryMetrics measures the
  // spline as it is: getTimeSum, checkRatio, checkFeasibility, getLength, getJerk, getMeanAndMaxVel / Acc.  Both return
  // false, and touch no output, when the call fails.
  bool adjustTime(const Eigen::MatrixXd& pos_ctrl, int degree, double dt, Eigen::VectorXd& knots, int ops,
                  const double* ratio_in, const TrajAdjust& cfg, TrajMetrics& out, Eigen::MatrixXd* samples);
  bool trajectoryMetrics(const Eigen::MatrixXd& pos_ctrl, int degree, double dt, const Eigen::VectorXd& knots,
                         const TrajAdjust& cfg, TrajMetrics& out);
  // selectBestTraj (planner_manager.cpp:476-482) over uniform splines (control points, knot span) of one degree: the index
  // of the smallest getJerk(), the smallest index on a tie, never a jerk that is not a number; -1: no candidate (or
  // the call failed).  All splines are measured in one device call and ranked there.
  int selectBestTraj(const std::vector<Eigen::MatrixXd>& pos_ctrl, int degree, const std::vector<double>& dt,
                     const TrajAdjust& cfg, std::vector<TrajMetrics>* all);

  // addition: FastPlannerManager::paramLocalTraj / reparamLocalTraj (planner_manager.cpp:605-634) on the device
  // (fuelmi_map_local_segments, include/fuelmi.h).  The state is what GlobalTrajData holds, as plain data: the
  // polynomial global trajectory (PolynomialTraj's segment times and coefficients, lowest power first), the uniform
  // local spline of this optimiser's degree (no rows: none yet) and the four times setGlobalTraj / setLocalTraj keep.
  struct GlobalTrajState {
    std::vector<double> seg_times;                  // [S]
    std::vector<double> coef;                       // [S][3][6]: segment, axis, power
    double global_duration = 0.0;
    Eigen::MatrixXd local_ctrl;                     // [n][3], or empty
    double local_knot_span = 0.0;
    double local_start_time = -1.0, local_end_time = -1.0, time_change = 0.0, last_time_inc = 0.0;
  };
  // what one call comes back with: the control points parameterizeToBspline returns, dt / duration, the boundary
  // derivatives (plan_data_.local_start_end_derivative_) and the sampled points; status is FUELMI_LOCALSEG_*
  struct LocalSegment {
    int status = 0, n_steps = 0, seg_num = 0;
    double segment_len = 0.0, dt = 0.0, duration = 0.0;
    Eigen::MatrixXd ctrl_pts;
    vector<Eigen::Vector3d> points, start_end_derivative;
  };
  // paramLocalTraj(start_t, dt, duration) with pp_.local_traj_len_ = radius and pp_.ctrl_pt_dist = dist_pt.
  // reparamLocalTraj(start_t, duration, dt) for every dt of `dts` in ONE device call: optimizeTopoBspline makes one
  // call per guide path, each with its own dt and therefore its own number of points.  Both return false, and touch no
  // output, when the call fails; a problem's own failure is its status.
  bool paramLocalTraj(const GlobalTrajState& state, double start_t, double radius, double dist_pt, LocalSegment& out);
  bool reparamLocalTraj(const GlobalTrajState& state, double start_t, double duration, const std::vector<double>& dts,
                        std::vector<LocalSegment>& out);

  // addition: the exact solve of the quadratic phases (fuelmi_map_solve_quadratic, include/fuelmi.h).  With the parameter
  // optimization/exact_quadratic set (default false: nothing changes), optimize() sends a cost mask without DISTANCE,
  // FEASIBILITY, VIEWCONS or MINTIME there -- the minimiser the phase is defined to reach instead of the iteration's best
  // of max_iteration_num evaluations -- and falls back to the iteration when the problem's status is FUELMI_QUAD_BOUNDED
  // or FUELMI_QUAD_DEGENERATE.  exact_status_ says what the last optimize() did: -1 the iteration alone, otherwise the
  // exact solve's status.
  // optimizeGuidePhase is the first phase of optimizeTopoBspline (plan_manage/src/planner_manager.cpp:584-588) for ALL
  // guide paths in one device call, each with its own number of control points (rows of ctrl_pts[i], knot span dts[i],
  // start / end states as setBoundaryStates takes them, guide[i] as setGuidePath takes it: rows - 2 bspline_degree
  // points).  ctrl_pts[i] is replaced where status[i] is FUELMI_QUAD_OK; the others are left for optimize().  Returns
  // false, and touches no output, when the call fails.
  bool exact_quadratic_ = false;
  int exact_status_ = -1;
  bool optimizeGuidePhase(std::vector<Eigen::MatrixXd>& ctrl_pts, const std::vector<double>& dts,
                          const std::vector<vector<Eigen::Vector3d>>& start, const std::vector<vector<Eigen::Vector3d>>& end,
                          const std::vector<vector<Eigen::Vector3d>>& guide, std::vector<int>& status,
                          std::vector<double>& cost);

  Eigen::MatrixXd getControlPoints();
  vector<Eigen::Vector3d> matrixToVectors(const Eigen::MatrixXd& ctrl_pts);

  // addition: one combineCost evaluation (variables in NLopt layout) on the device
  void combineCost(const std::vector<double>& x, std::vector<double>& grad, double& cost);

  // diagnostics the reference exposes as public members
  double comb_time;
  ros::Time time_start_;
  vector<double> vec_cost_, vec_time_;
  void getCostCurve(vector<double>& cost, vector<double>& time) {
    cost = vec_cost_;
    time = vec_time_;
  }

  EIGEN_MAKE_ALIGNED_OPERATOR_NEW

private:
  bool isQuadratic();
  bool solveExact();  // optimize()'s exact route: true when it took the problem

  // environment and parameters
  shared_ptr<EDTEnvironment> edt_environment_;
  fuelmi_bspline_cfg cfg_;
  int bspline_degree_, algorithm1_, algorithm2_;
  int max_iteration_num_[4];
  double max_iteration_time_[4];
  bool dynamic_;
  double start_time_;

  // the problem being solved
  Eigen::MatrixXd control_points_;
  double knot_span_, time_lb_, pt_dist_;
  int cost_function_, dim_, order_, point_num_, variable_num_, max_num_id_, max_time_id_;
  bool optimize_time_;
  vector<Eigen::Vector3d> start_state_, end_state_, guide_pts_, waypoints_;
  vector<int> waypt_idx_;
  ViewConstraint view_cons_;

  // result of the last solve
  std::vector<double> best_variable_;
  double min_cost_;
  int iter_num_;
};
}  // namespace fast_planner
#endif
