// stand-in (tests/golden/make_heading_golden.py only): heading_planner.cpp includes the header and uses nothing of it
#ifndef HEADING_GOLDEN_EXTRACT_INDICES_H_
#define HEADING_GOLDEN_EXTRACT_INDICES_H_
#endif
