// mesh_key.h — keys in mesh units (MAC_OPT_MESH_KEYS), shared by host and device code: the poll
// chains inline these, mac_diag_mesh_key exports them for the CPU tests (tests/test_mesh_keys_host.py).
//
// On a generated poll with a mesh, candidate k's value of polled variable v is x + d or x - d with
// x = xinc[v], d = fl(g[v] * (double)L) and L the integer draw (k_prep.h CandSrc::step_m, get_m).
// x - d == x + (-d) and -fl(g * L) == fl(g * (-L)) hold exactly, so with the signed draw m = +-L the
// one decode x + g * (double)m (one product, one add, no contraction) is the candidate's double bit
// for bit. (One corner is not covered by the identities: L = 0 has no sign as an integer, so on a
// -0.0 incumbent the minus candidate -0.0 - 0.0 = -0.0 is not the decode -0.0 + g * 0 = +0.0. The
// check below refuses that word like any other that does not reproduce its double.) A mesh key is disk i's triple (m_x, m_y, m_r) in the 11 + 11 + 10-bit word of k_prep.h
// key_pack, its base the incumbent and its scale the disk's three granularities; a held variable
// has m = 0. A word is written only when the decode reproduces all three doubles (mesh_key_exact:
// it catches m = 0 on a -0.0 incumbent, whose decode is +0.0), so equal words mean equal disks.
#pragma once

#include <stdint.h>

#include "predicate.h"

#pragma clang fp contract(off)

namespace mac {

constexpr uint32_t kMeshKeyEsc = 0x200u << 22;   // k_prep.h kKeyEsc: the r field -512, never packed
constexpr double kMeshKeyLimXY = 1023.0, kMeshKeyLimR = 511.0;

// the signed draw e (an integer-valued double, 0.0 for a held variable) as a key field: false when
// it is no integer of at most lim in magnitude (NaN: false)
MAC_HD bool mesh_key_field(double e, double lim, int& m)
{
    if (!(e >= -lim && e <= lim)) return false;
    m = (int)e;
    return (double)m == e;
}

// the candidate's double from the incumbent's x, the variable's granularity g and the signed draw
MAC_HD double mesh_key_decode(double x, double g, double m) { return x + g * m; }

MAC_HD bool mesh_key_exact(double x, double g, int m, double v)
{
    return __builtin_bit_cast(uint64_t, mesh_key_decode(x, g, (double)m)) == __builtin_bit_cast(uint64_t, v);
}

// the word of (m_x, m_y, m_r); false (and the escape word) when a draw is past its field:
// |m_x|, |m_y| > 1023 or |m_r| > 511 (-512 is the escape pattern's r field)
MAC_HD bool mesh_key_pack(int mx, int my, int mr, uint32_t& w)
{
    const bool fits = mx >= -1023 && mx <= 1023 && my >= -1023 && my <= 1023 && mr >= -511 && mr <= 511;
    w = fits ? ((uint32_t)mx & 0x7FFu) | (((uint32_t)my & 0x7FFu) << 11) | (((uint32_t)mr & 0x3FFu) << 22)
             : kMeshKeyEsc;
    return fits;
}

MAC_HD void mesh_key_unpack(uint32_t w, int& mx, int& my, int& mr)
{
    mx = (int)(w << 21) >> 21;
    my = (int)(w << 10) >> 21;
    mr = (int)w >> 22;
}

// One field of a word under construction (q = 0, 1, 2: x, y, r) from the variable's signed draw e:
// ORs the field into w; false when the draw does not pack or its decode is not v bit for bit.
MAC_HD bool mesh_key_put(uint32_t& w, int q, double x, double g, double e, double v)
{
    int m = 0;
    const bool ok = mesh_key_field(e, q == 2 ? kMeshKeyLimR : kMeshKeyLimXY, m) && mesh_key_exact(x, g, m, v);
    w |= q == 0 ? ((uint32_t)m & 0x7FFu) : q == 1 ? ((uint32_t)m & 0x7FFu) << 11 : ((uint32_t)m & 0x3FFu) << 22;
    return ok;
}

}  // namespace mac
