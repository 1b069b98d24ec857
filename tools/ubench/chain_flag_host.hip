// Host check of the chained accumulator's flag identity (pg_common.h, "chained filter MFMAs"), no GPU: for EVERY
// triple of filter results in [PG_SIG_D_MIN, PG_SIG_D_MAX]^3 - sequential f32 accumulation from 2.0, as the matrix core
// chains them - the value is the exact one, (bits & PG_CHAIN_FLAGS) != 0 <=> some result is negative, and the per-field
// flags name a superset of the negative fields.  The same for chains of two and of one (unused fields 0).
//   hipcc --cuda-host-only -O2 chain_flag_host.hip -o chain_flag_host && ./chain_flag_host
#include "../../prograph_amd/csrc/pg_common.h"
#include <cstdio>
#include <cstring>

int main() {
  long long n = 0, badValue = 0, badFlag = 0, badField = 0;
  for (int d2 = PG_SIG_D_MIN; d2 <= PG_SIG_D_MAX; ++d2)
    for (int d1 = PG_SIG_D_MIN; d1 <= PG_SIG_D_MAX; ++d1)
      for (int d0 = PG_SIG_D_MIN; d0 <= PG_SIG_D_MAX; ++d0) {
        const float x = pg_chain_value(d0, d1, d2);
        const long long S = d0 + 256ll * d1 + 65536ll * d2;
        const float want = (float)((1ll << 23) + S) * 0x1p-22f;        // an integer below 2^24: exact
        u32 b, w;
        memcpy(&b, &x, 4);
        memcpy(&w, &want, 4);
        ++n;
        badValue += b != w;
        badFlag += (pg_chain_flag(b) != 0u) != (d0 < 0 || d1 < 0 || d2 < 0);
        badField += (d0 < 0 && !(b & 0x20000080u)) || (d1 < 0 && !(b & 0x20008000u)) || (d2 < 0 && !(b & 0x20000000u));
      }
  printf("%lld triples in [%d, %d]^3: %lld values wrong, %lld flags wrong, %lld negative fields not named\n", n, PG_SIG_D_MIN,
         PG_SIG_D_MAX, badValue, badFlag, badField);
  return (badValue || badFlag || badField || n != 227ll * 227 * 227) ? 1 : 0;
}
