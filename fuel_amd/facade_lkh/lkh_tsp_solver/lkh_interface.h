// lkh_tsp_solver/lkh_interface.h -- drop-in for the header of the reference's TSP solver package
// (fuel_planner/utils/lkh_tsp_solver/include/lkh_tsp_solver/lkh_interface.h): the one entry point the exploration
// manager calls (fast_exploration_manager.cpp:378), implemented by libfuelmi_lkh.so on the device ATSP solver of
// libfuelmi.so (include/fuelmi.h "Global tour").  See INTEGRATION.md.
#ifndef _LKH_INTERFACE_H
#define _LKH_INTERFACE_H

// Reads the LKH parameter file par_file and writes the tour of its problem.  Returns 0, or nonzero with a message on
// stderr after removing the tour files it names (a caller that reads the tour file anyway finds none).
int solveTSPLKH(const char* input_file);

#endif
