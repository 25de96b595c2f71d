// The statements of rsd::jacobi3 and rsd::jacobi3_exact (device_math.h), which include this file
// inside their bodies: the same text compiled once with the translation unit's contraction and
// once under `#pragma clang fp contract(off)`.  A pragma is lexical, so a template or an inlined
// call cannot make that choice; a second copy of the loop could drift.  No include guard.
//
// In scope: double (&A)[9], the symmetric matrix, row-major, destroyed; double (&V)[9].
#pragma unroll
for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
for (int sweep = 0; sweep < 30; ++sweep) {
  const double off = A[1] * A[1] + A[2] * A[2] + A[5] * A[5];
  const double dia = A[0] * A[0] + A[4] * A[4] + A[8] * A[8];
  if (!(off > 1e-30 * dia)) break;
#pragma unroll
  for (int pq = 0; pq < 3; ++pq) {
    const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
    const double apq = A[p * 3 + q];
    if (apq == 0.0) continue;
    const double th = (A[q * 3 + q] - A[p * 3 + p]) / (2.0 * apq);
    const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // columns p, q
      const double akp = A[k * 3 + p], akq = A[k * 3 + q];
      A[k * 3 + p] = c * akp - s * akq;
      A[k * 3 + q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // rows p, q
      const double apk = A[p * 3 + k], aqk = A[q * 3 + k];
      A[p * 3 + k] = c * apk - s * aqk;
      A[q * 3 + k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double vkp = V[k * 3 + p], vkq = V[k * 3 + q];
      V[k * 3 + p] = c * vkp - s * vkq;
      V[k * 3 + q] = s * vkp + c * vkq;
    }
  }
}
