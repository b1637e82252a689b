"""MI355X-native scan matching + occupancy mapping for the course_agv SLAM stack.

Drop-in replacements, on hand-written gfx950 HIP kernels behind a C ABI
(include/slam_hip.h, csrc/), for the per-scan hot path of
zjwzcx/A-2D-LiDAR-based-SLAM-System-for-Wheeled-Mobile-Robots:

    ICP        process / findNearest / getTransform / laserToNumpy / laserCallback / publishResult
    Mapping    update -> pmap; raycast / score_scan read the map along rays (batched: DeviceGrid.raycast /
               .score, grid_raycast_host / grid_score_host); distance_field / match_scan: where a scan fits
               the map best (batched: DeviceGrid.distance_field / .match, grid_distance_field_host /
               grid_match_host, match_pose); locate_scan: where in the whole map a scan was taken (batched:
               DeviceGrid.locate, grid_locate_host, locate_rotations, locate_pose; MCL.init_global starts from it);
               frontiers / next_goal: where to go next to see more of the map - clustered frontier cells, one goal per
               cluster (batched: DeviceGrid.frontiers, grid_frontiers_host, frontier_points; GridSLAM / DeviceGridSLAM
               .frontiers on the best particle's map); travel_field / travel_path / next_goal(by="travel"): what it
               costs to drive to every cell, the way there, and the frontier that is nearest to drive to (batched:
               DeviceGrid.travel, grid_travel_host; DeviceGridSLAM.travel / .next_goals); view_gain /
               next_goal(by="gain"): the cells a scan from a pose would reveal, and the frontier that reveals the most
               unknown cells per unit of travel (batched: DeviceGrid.view_gain, grid_view_gain_host, view_poses,
               gain_goal; GridSLAM / DeviceGridSLAM .view_gain, DeviceGridSLAM.next_goals(by="gain")); refine_scan /
               match_scan(refine=k): a matched pose moved below the cell by damped Gauss-Newton steps on the smooth
               distance field, with the 3 x 3 normal matrix of the fit (batched: DeviceGrid.refine, grid_refine_host,
               refine_normal; include/slam_refine.h)
    bresenham  (start, end).path
    SLAM_EKF   laserCallback glue (scan matching + map building); landmarks=True: the whole W12
               node with Extraction and the landmark EKF on the host; batched on the device
               as DeviceNodeReplay / node_replay_host, landmarks_host, ekf_lm_host
    Localization  updateMap / laserEstimation / calc_map_observation (scan-to-map, W9); the whole
               W9 node batched on the device as DeviceLocalizationReplay / loc_replay_host
    MCL        Monte Carlo localisation on the map's distance field: one filter on a Mapping; batched and
               device-resident as DeviceMCL, on NumPy arrays as mcl_weigh_host / mcl_resample_host
    GridSLAM   grid FastSLAM: a particle filter whose every particle builds its own map, and the maps follow the
               resampling (in place; only the maps of particles that died are copied); batched and device-resident
               as DeviceGridSLAM, on NumPy arrays as mcl_weigh_host(own_maps=True) / mcl_settle_host /
               grid_copy_maps_host / grid_update_particles_host (DeviceGrid.copy_maps / .update_particles)
    ScanTracker  scan-to-map tracking: every scan matched against the map so far, refined below the cell and, behind a
               keyframe gate, integrated - one call per scan stream (include/slam_track.h); batched and
               device-resident as DeviceTracker, on NumPy arrays as track_host (track_rotations, new_state)
    dwa        dwa_control / Config / RobotType (course_agv_nav DWA local planner), batched as
               DeviceDWA / dwa_batch_host; LocalPlanner: the local planner node without ROS
    global_planner  find_path(...).start_find() / GlobalPlanner (course_agv_nav A*), batched as
               DeviceAStar / astar_host

plus the batched forms used by bench.py (``replay``), the maps and their queries (``grid``: DeviceGrid and every
grid_*_host) and the multi-GPU sharding helper (``dist``).  Importing the package never computes anything; every operator raises if
libslamhip.so or the GPU is missing (there is no CPU implementation in the product).
"""
from . import _abi, dist, param, synthetic
from ._abi import Context, LibraryMissing, SlamError, default_context
from ._abi import TRAVEL_DIAGONAL, TRAVEL_STRAIGHT, TRAVEL_TRIPS
from ._abi import RAY_BAD, RAY_BLOCKED, RAY_CLASSES, RAY_EMPTY, RAY_FREE, RAY_HIT, RAY_NAMES, RAY_OUT, RAY_UNKNOWN
from ._abi import VIEW_COUNTS, VIEW_FREE, VIEW_OCCUPIED, VIEW_OPEN, VIEW_UNKNOWN
from ._abi import REFINE_BAD_POSE, REFINE_NO_MAP, REFINE_NORMAL_LEN, REFINE_OK
from ._abi import TRACK_INTEGRATED, TRACK_LOST, TRACK_MATCHED, TRACK_REFINED
from . import dwa
from .bresenham import bresenham, rasterize
from .dwa import DeviceDWA, dwa_batch_host, dwa_control
from .ekf_lm import EKF
from .extraction import Extraction, LandMarkSet
from . import global_planner
from .global_planner import DeviceAStar, GlobalPlanner, astar_host, find_path, inflate_host
from .icp import ICP, scan_to_pc
from .local_planner import LocalPlanner
from .localization import Localization
from .loc_replay import DeviceLocalizationReplay, loc_replay_host
from .mapping import Mapping
from .mcl import MCL, MCL_DEAD, DeviceMCL, mcl_resample_host, mcl_settle_host, mcl_weigh_host, mcl_weight_table
from .node_replay import DeviceNodeReplay, ekf_lm_host, landmarks_host, node_replay_host
from .grid import DeviceGrid, grid_raycast_host, grid_score_host
from .grid import grid_distance_field_host, grid_match_host, match_pose, match_rotations
from .grid import grid_copy_maps_host, grid_update_particles_host
from .grid import grid_locate_host, locate_pose, locate_rotations
from .grid import frontier_points, grid_frontiers_host, grid_travel_host
from .grid import gain_goal, grid_view_gain_host, view_poses, view_tables
from .grid import grid_refine_host, refine_normal
from .replay import DeviceReplay, icp_batch_host, particles_host, prior_matrices, replay_host
from .grid_slam import DeviceGridSLAM, GridSLAM
from .slam_ekf import SLAM_EKF
from .tracker import DeviceTracker, ScanTracker, new_state, track_host, track_rotations
from .synthetic import LaserScan

__all__ = ["ICP", "Mapping", "Localization", "EKF", "Extraction", "LandMarkSet", "bresenham", "rasterize", "SLAM_EKF", "LaserScan", "Context", "default_context",
           "DeviceGrid", "DeviceReplay", "replay_host", "icp_batch_host", "particles_host", "prior_matrices", "scan_to_pc", "SlamError",
           "LibraryMissing", "param", "synthetic", "dwa", "dwa_control", "DeviceDWA", "dwa_batch_host", "LocalPlanner",
           "global_planner", "find_path", "GlobalPlanner", "DeviceAStar", "astar_host", "inflate_host",
           "DeviceNodeReplay", "node_replay_host", "landmarks_host", "ekf_lm_host",
           "DeviceLocalizationReplay", "loc_replay_host", "grid_raycast_host", "grid_score_host",
           "grid_distance_field_host", "grid_match_host", "match_pose", "match_rotations",
           "grid_locate_host", "locate_pose", "locate_rotations", "grid_frontiers_host", "frontier_points", "grid_travel_host",
           "TRAVEL_STRAIGHT", "TRAVEL_DIAGONAL", "TRAVEL_TRIPS",
           "MCL", "DeviceMCL", "MCL_DEAD", "mcl_weight_table", "mcl_weigh_host", "mcl_resample_host",
           "GridSLAM", "DeviceGridSLAM", "mcl_settle_host", "grid_copy_maps_host", "grid_update_particles_host",
           "RAY_EMPTY", "RAY_HIT", "RAY_BLOCKED", "RAY_FREE", "RAY_UNKNOWN", "RAY_OUT", "RAY_BAD", "RAY_CLASSES", "RAY_NAMES",
           "grid_view_gain_host", "view_poses", "view_tables", "gain_goal", "VIEW_UNKNOWN", "VIEW_FREE", "VIEW_OCCUPIED", "VIEW_OPEN", "VIEW_COUNTS",
           "grid_refine_host", "refine_normal", "REFINE_OK", "REFINE_BAD_POSE", "REFINE_NO_MAP", "REFINE_NORMAL_LEN",
           "DeviceTracker", "ScanTracker", "track_host", "track_rotations", "new_state",
           "TRACK_MATCHED", "TRACK_REFINED", "TRACK_INTEGRATED", "TRACK_LOST"]
