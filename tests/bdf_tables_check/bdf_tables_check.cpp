// TEST INFRASTRUCTURE ONLY (tests/test_bdf_tables.py).  Prints the Bdf::_new tables of diffsol_amd/csrc/dsh_bdf_tables.hpp twice as 64-bit patterns: "run"
// lines from bdf_new_tables() executed as compiled code, the way the host set-up of the device-resident BDF fills AdaptiveConsts (called through a volatile
// pointer and built without optimisation, so that the arithmetic is the machine's), and "const" lines from kBdfTables, the constant-evaluated table whose
// entries the per-order step bodies of the lock-step fast kernel carry as literals.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "dsh_bdf_tables.hpp"

static void print(const char* tag, const dsh::BdfTables& T) {
  const double* tabs[3] = {T.alpha, T.gamma, T.ec2};
  const char* names[3] = {"alpha", "gamma", "ec2"};
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < 6; ++i) {
      uint64_t u;
      std::memcpy(&u, &tabs[k][i], 8);
      std::printf("%s %s %d %016llx\n", tag, names[k], i, (unsigned long long)u);
    }
}

int main() {
  dsh::BdfTables (*volatile fill)() = &dsh::bdf_new_tables;
  const dsh::BdfTables run = fill();
  static constexpr dsh::BdfTables konst = dsh::kBdfTables;
  static_assert(konst.gamma[1] == 1.0 && konst.gamma[2] == 1.5, "the table is constant-evaluated");
  print("run", run);
  print("const", konst);
  return 0;
}
