// Host build of launch_plan.hpp alone (test-only; never linked into the product): sim.cpp's plan exports without the field and
// curve code, so that a test next to a GPU run can ask the launcher's plan from a library that builds in a second.
#include <cstddef>
#include <cstdint>
#include "launch_plan.hpp"
using namespace d377;

extern "C" {
#include "launch_plan_sim.inc"
}
