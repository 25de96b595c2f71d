"""MI355X-native RANSAC-F / PnP hot path of bioengstrom/tsbb15-3d-reconstruction-project.

Drop-in modules mirroring the reference surface:
  tsbb15_amd.lab3    fmatrix_stls, fmatrix_residuals, homog
  tsbb15_amd.fun     getFFromLabCode, ransac_f
  tsbb15_amd.ransac  calc_p, calc_r, gen_rnd_indices, norm_p, cart, dpp, dpp_squared,
                     calc_y_prim, ransac_robust
  tsbb15_amd.pnp     p3p, pnp_minimize
  tsbb15_amd.cv      solvePnPRansac, Rodrigues (the tables.py:141-145 call site)
  tsbb15_amd.evaluation  mesh_distance, compare_meshes, camera_errors (the step evaluation.py
                     names: accuracy and completeness of a mesh, errors of the cameras)
  tsbb15_amd.tracking  track, track_sequence, Correspondences (the track array of
                     imgdata/points.txt from images: a pyramidal Lucas-Kanade tracker)
Compute runs in lib/librsamd.so (HIP, gfx950) through ctypes; there is no CPU fallback.
"""
__version__ = "0.1.0"
