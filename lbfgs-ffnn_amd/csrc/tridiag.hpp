// Eigenvalues of a symmetric tridiagonal matrix on the host (tridiag.cpp): what turns a Lanczos run's alpha and beta
// into Ritz values and quadrature weights. No device code and no device header.
#pragma once

namespace lbf {

// T = tridiag(beta[0..m-2]; alpha[0..m-1]; beta[0..m-2]), m >= 1; a zero beta (decoupled blocks) is legal. Implicit
// QL with Wilkinson shifts in fp64. theta[m]: the eigenvalues, ascending. first_sq (nullable, m): the squared first
// component of each normalised eigenvector, in theta's order. vecs (nullable, m * m): vecs[i * m + k] is component i
// of the eigenvector of theta[k]. Returns false when an eigenvalue does not converge in 60 sweeps (a non-finite
// entry); the outputs are then unspecified.
bool tridiag_eig(int m, const double *alpha, const double *beta, double *theta, double *first_sq, double *vecs);

} // namespace lbf
