// mvx_box_cull.inc - the radius an atom is culled with and the box cull itself (rule step 1), as one piece of text for the two
// places that apply it: prep_atom (mvx_device.h: the pre-pass of every forward and backward call) and the view selection
// (mvx_views.hip), which keeps exactly the atoms that pass here. Included inside a function body that has in scope
//   A (PrepArgs), a (the atom's index), p[3] (its position after centring / transform), f64 (A.precision == 64),
//   lb / ub (-half / +half of the grid), rmax32 / rmax64 (max channel radius, RAD_CHANNEL_FEATURES only), and the
//   declarations of r32, rc, rwin, r64 (the radii the caller goes on with);
// it declares `keep` (false: outside the box widened by the cull radius, or a type outside [0, C)) and `type`.
    bool keep = true;
    int32_t type = 0;
    if (A.types) {
        type = A.types[a];
        if (type < 0 || type >= A.C) keep = false; // never index radii / channels out of range
    }
    if (A.radii_src == RAD_SCALAR) {
        rc = A.radius_scalar;
        r32 = (float)A.radius_scalar;
        r64 = A.radius_scalar;
        rwin = f64 ? r64 : (double)r32;
        for (int i = 0; i < 3; ++i) keep = keep && (p[i] > lb - rc) && (p[i] < ub + rc); // numpy/voxelizer.py:487-488
    } else if (A.radii_src == RAD_CHANNEL_FEATURES) {
        double lo, hi;
        if (f64) { // np.float64 scalar: plain float64 arithmetic
            r64 = rmax64;
            r32 = (float)r64;
            rc = rwin = r64;
            lo = lb - r64;
            hi = ub + r64;
        } else {
            const float rmax = rmax32;
            r32 = rmax;
            rc = rwin = (double)rmax;
            // np.float32 scalar: (python float -/+ float32) is evaluated in float32 (NEP 50), numpy/voxelizer.py:138
            lo = (double)((float)lb - rmax);
            hi = (double)((float)ub + rmax);
        }
        for (int i = 0; i < 3; ++i) keep = keep && (p[i] > lo) && (p[i] < hi);
    } else {
        const int64_t ri = (A.radii_src == RAD_ATOM) ? a : (keep ? (int64_t)type : -1); // numpy/voxelizer.py:284-285
        if (f64) {
            r64 = ri >= 0 ? static_cast<const double *>(A.radii)[ri] : 0.0;
            r32 = (float)r64;
            rc = rwin = r64;
        } else {
            r32 = ri >= 0 ? static_cast<const float *>(A.radii)[ri] : 0.0f;
            rc = rwin = (double)r32;
        }
        for (int i = 0; i < 3; ++i) keep = keep && (p[i] + rc > lb) && (p[i] - rc < ub); // numpy/voxelizer.py:491-492
    }
