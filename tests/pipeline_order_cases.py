"""Which call may follow a pipelined replay, and which test says so (test infrastructure only).

The "pipeline" option of a context runs slam_replay_dev with a map as three stages on three streams.  include/slam_hip.h
promises that the results of the later stages (poses_out, pmap_dev) are visible "to any later call on this context".
Every ``slam_*_dev`` entry point - and the few others that hand out or read back what the stages write - is either a
LEG of tests/test_gpu_pipeline_order.py (``def leg_<name>``) or EXEMPT here with its reason.  tests/test_pipeline_order_cases.py
holds the table against the header, so an entry point cannot be added without a decision about its ordering.

A leg is ``name: (entry point, what it takes from the pipelined stages)``:
    grid    the counters of the map stage, read or written
    M       the int8 pmap that slam_grid_finalize_dev wrote on the map stream
    P-in    poses_out of the replay, read
    P-out   a buffer that the ray cast of the map stage is still reading, written
    stream  slam_stream_order(stream, 0), then the caller's own stream reads P and M"""

LEGS = {
    # the grid, read
    "raycast": ("slam_grid_raycast_dev", "grid"),
    "scan_score": ("slam_grid_scan_score_dev", "grid"),
    "view_gain": ("slam_grid_view_gain_dev", "grid"),
    "distance_field": ("slam_grid_distance_field_dev", "grid"),
    "match": ("slam_grid_match_dev", "grid"),
    "locate": ("slam_grid_locate_dev", "grid"),
    "frontiers": ("slam_grid_frontiers_dev", "grid"),
    "travel": ("slam_grid_travel_dev", "grid"),
    "mcl_weigh": ("slam_mcl_weigh_dev", "grid"),
    "mcl_weigh_maps": ("slam_mcl_weigh_maps_dev", "grid"),
    "copy_maps": ("slam_grid_copy_maps_dev", "grid"),
    # the grid, written
    "update": ("slam_grid_update_dev", "grid"),
    "update_scans": ("slam_grid_update_scans_dev", "grid"),
    "update_particles": ("slam_grid_update_particles_dev", "grid"),
    # the grid, handed out or read back
    "counters": ("slam_grid_counters_dev", "grid"),
    "live_pmap": ("slam_grid_live_pmap", "grid"),
    "occupancy_data": ("slam_grid_occupancy_data", "grid"),
    "visits": ("slam_grid_visits", "grid"),
    # M
    "astar": ("slam_astar_dev", "M"),
    "astar_inflate": ("slam_astar_inflate_dev", "M"),
    "map_obstacles": ("slam_map_obstacles_dev", "M"),
    # P, read
    "pose_compose_pose0": ("slam_pose_compose_dev", "P-in"),
    "virtual_scan": ("slam_virtual_scan_dev", "P-in"),
    "map_observation": ("slam_map_observation_dev", "P-in"),
    "mcl_settle_src": ("slam_mcl_settle_dev", "P-in"),
    "mcl_resample_poses": ("slam_mcl_resample_dev", "P-in"),
    "particles_pose_prev": ("slam_particles_dev", "P-in"),
    "raycast_poses": ("slam_grid_raycast_dev", "P-in"),
    "view_gain_poses": ("slam_grid_view_gain_dev", "P-in"),
    "replay_chain_map": ("slam_replay_dev", "P-in"),
    "replay_chain_no_map": ("slam_replay_dev", "P-in"),
    "ekf_lm": ("slam_ekf_lm_dev", "P-in"),
    "node_replay": ("slam_node_replay_dev", "P-in"),
    "loc_replay": ("slam_loc_replay_dev", "P-in"),
    # P, written while the map stage reads it
    "pose_compose_out": ("slam_pose_compose_dev", "P-out"),
    "mcl_settle_out": ("slam_mcl_settle_dev", "P-out"),
    # the caller's own stream
    "stream_order": ("slam_stream_order", "stream"),
}

# Entry points without a leg.  The first three are the pipeline's own stages: a join in them would undo the overlap the
# option is for (the piped slam_replay_dev is exempt as a CONSUMER of the join; the replay_chain legs follow it with a
# second and a third replay).  The others take no map and join the internal streams at their head exactly as the legs
# of their kind do (streams_on_main, csrc/slam_abi.hip).  No argument of theirs has the type of a stage result -
# poses_out is float64 [.][3] poses and pmap_dev an int8 map - so a leg would have to feed them bytes that mean something
# else.  (The three nodes that take a start pose - the landmark filter, the landmark node and the localization node -
# have their legs above: x0 / pose0 is the last row of the piped replay's poses_out.)
EXEMPT = {
    "slam_replay_dev[piped]": "the pipeline itself: scan matching | pose composition | map stage, ordered by its own events",
    "slam_grid_reset": "first piece of the map stage: runs on the map stream, behind the previous map stage",
    "slam_grid_finalize_dev": "last piece of the map stage: runs on the map stream, behind the ray cast",
    "slam_scan_to_points_dev": "reads float32 ranges and beam tables only",
    "slam_scan_to_points_f64_dev": "reads float64 ranges and beam tables only",
    "slam_nn_dev": "reads two point clouds only",
    "slam_kabsch2d_dev": "reads two point clouds only",
    "slam_icp_batch_dev": "reads point clouds and 2 x 3 priors only",
    "slam_dwa_dev": "reads [B][5] planner states, goals and obstacle points only",
    "slam_dwa_scans_dev": "reads [B][5] planner states, goals and float32 ranges only",
    "slam_landmarks_dev": "reads float32 ranges and beam tables only",
}


def dev_entry_points(header_text):
    """Every function named slam_*_dev that the header declares (comments removed first)."""
    import re
    text = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    return sorted(set(re.findall(r"\b(slam_[a-z0-9_]+_dev)\s*\(", text)))
