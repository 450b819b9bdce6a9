// pnp.cpp -- see pnp_problem.h.  Drop-in for pvio/src/pvio/estimation/pnp.cpp (compiled against the reference's headers
// inside the PVIO tree, host_seam.h): flattens `frame` against `map` into a PnpProblem and hands it to solve_pnp (pnp_solve.cpp).
#include "host_seam.h"
#include "flat_layout.h"
#include "pnp_problem.h"

#include <cmath>
#include <cstring>
#include <limits>

namespace pvio {

void visual_inertial_pnp(Map *map, Frame *frame, Config *config, bool use_inertial) {
    Frame *last = map->last_frame();
    PnpProblem pb;
    flat::put_extrinsic(pb.cam, frame->camera), flat::put_extrinsic(pb.imu, frame->imu);
    flat::put_sqrt_inv_cov(pb.sqrt_inv_cov, frame->sqrt_inv_cov);
    pb.use_inertial = use_inertial;
    flat::put_state(pb.last_state, last), flat::put_extrinsic(pb.last_imu, last->imu);
    if (use_inertial) flat::put_preintegration(pb.delta, pb.sqrt_inv_cov_imu, pb.jac, frame->preintegration);
    // Residual blocks in the reference's order (pnp.cpp:55-93): keypoint index order, plane-point and anchored factors
    // interleaved.  PnpProblem keeps the two kinds in separate lists, i.e. the cost sums them in another order -- a
    // rounding-level difference, like the landmark-major order of the window solve.
    for (size_t i = 0; i < frame->keypoint_num(); ++i) {
        Track *track = frame->get_track(i);
        if (!track) continue;
        if (!track->has_keypoint(last)) continue;
        if (!track->flag(TrackFlag::TF_VALID)) continue;
        const vector<2> &zt = frame->get_keypoint(i);
        if (track->flag(TrackFlag::TF_PLANE)) { // PVIO_ENABLE_PLANE_CONSTRAINT (ON by default, CMakeLists.txt:10): pnp.cpp:61-88
            // "find best plane via reprojection error": the reference never updates max_rpe, so every plane that is not
            // parallel to the anchor's viewing ray and whose reprojection error is below DBL_MAX replaces the previous
            // choice -- the LAST such plane of the map wins.  Reproduced as is.
            bool have = false;
            vector<3> best_plane_point;
            const double max_rpe = std::numeric_limits<double>::max();
            const auto ref = track->first_keypoint();
            const PoseState cam = ref.first->get_pose(ref.first->camera);
            const vector<3> direction = cam.q * ref.first->get_keypoint(ref.second).homogeneous();
            for (size_t j = 0; j < map->plane_num(); ++j) {
                Plane *plane = map->get_plane(j);
                if (plane->is_parallel(direction)) continue;
                const vector<3> plane_point = plane->cast_to_point(cam.p, direction);
                const double rpe = PlaneExtractor::compute_reprojection_error(map, track, plane_point);
                if (rpe < max_rpe) best_plane_point = plane_point, have = true;
            }
            // (with no admissible plane the reference hands an uninitialized point to the factor; here the keypoint is left out)
            if (have) {
                PnpPointFactor f;
                for (int k = 0; k < 3; ++k) f.point[k] = best_plane_point[k];
                f.z_tgt[0] = zt[0], f.z_tgt[1] = zt[1];
                pb.point_factors.push_back(f);
            }
            continue;
        }
        const auto anchor = track->first_keypoint();
        PnpFactor f;
        flat::put_state(f.anchor_state, anchor.first), flat::put_extrinsic(f.anchor_cam, anchor.first->camera);
        const vector<2> &zr = anchor.first->get_keypoint(anchor.second);
        f.z_ref[0] = zr[0], f.z_ref[1] = zr[1], f.z_tgt[0] = zt[0], f.z_tgt[1] = zt[1];
        f.inv_depth = track->landmark.inv_depth;
        pb.factors.push_back(f);
    }
    double x[16];
    flat::put_state(x, frame);
    solve_pnp(pb, x, (int)config->solver_iteration_limit());
    flat::write_back_state(x, frame, use_inertial);
}

} // namespace pvio
