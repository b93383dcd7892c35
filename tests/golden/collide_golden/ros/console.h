// ros/console.h -- the ROS_* macros come with the ros/ros.h stand-in of compat/
#include <ros/ros.h>
