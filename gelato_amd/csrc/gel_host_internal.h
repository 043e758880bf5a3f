// gel_host_internal.h -- what more than one of the host files gel_host*.hip needs and no HIP call is behind, and nothing else (the
// handle and what makes HIP calls: gel_host_handle.h, which includes this header).  Nothing declared here is part of the library's
// C surface (include/gelato_amd.h): the functions live in namespace gelhost and the whole header has hidden visibility, so that
// none of them becomes a dynamic symbol.
#pragma once
#include <string>
#include <vector>

#include "../../include/gelato_amd.h"

#pragma GCC visibility push(hidden)

namespace gelhost {

// sets the calling thread's message (gel_last_error) and returns code; defined in gel_host.hip beside the message itself
int fail(int code, const std::string& msg);

// the extended-precision generators (gel_host_lgr.hip)
typedef long double ld;
int lgr_nodes_ld(int n, std::vector<ld>& tau);                                      // flipped LGR nodes, ending at +1; -1 when n < 2
int lgr_diffmat_ld(int n, std::vector<double>& D, std::vector<double>& tau_out);    // D [n][n + 1] on [-1, tau], and tau
std::vector<ld> bary_weights(const std::vector<ld>& t);
// the Lagrange basis of support t (weights w) at z, second barycentric form; exactly 1 / 0 at a support point
void lagrange_row(const std::vector<ld>& t, const std::vector<ld>& w, ld z, ld* out);
// sigma [P], Lx [P][n+1], Lu [P][n], I [P][P] (row-major, P = n + 1) of a phase whose collocation points are tau [n]
int mesh_matrices_ld(const std::vector<double>& tau, std::vector<double>& out);

}  // namespace gelhost

#pragma GCC visibility pop
