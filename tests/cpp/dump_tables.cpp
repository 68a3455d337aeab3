// dump_tables.cpp -- writes work_plan.h's build_tables() (the MFMA tables an engine uploads) to
// stdout, for tests that check properties of the table values in Python
// (tests/test_phase_a_convert_cpu.py).
#include <cstdio>

#include "work_plan.h"

int main() {
  const std::vector<uint8_t> t = mipgpu::build_tables();
  return fwrite(t.data(), 1, t.size(), stdout) == t.size() ? 0 : 1;
}
