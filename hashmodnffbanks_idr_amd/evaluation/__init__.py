"""Evaluation of a reconstructed mesh and of rendered views on the device (reference: code/evaluation)."""
from .chamfer import dtu_chamfer, load_dtu_scan, mesh_chamfer, mesh_to_mesh  # noqa: F401
from .color import ColorStats, color_mesh, color_mesh_for_dataset  # noqa: F401
from .cull import CullStats, cull_mesh, cull_mesh_for_dataset, view_projections  # noqa: F401
from .images import evaluate_views, render_view, view_metrics  # noqa: F401
from .mesh_views import MeshViews, evaluate_mesh_views, render_mesh  # noqa: F401
from .mesh_rays import DepthAgreement, cast_camera_rays, depth_agreement  # noqa: F401
from .mesh_sdf import SdfAgreement, mesh_sdf_agreement, sdf_agreement, volume_iou  # noqa: F401
from .texture import TextureStats, texture_mesh, texture_mesh_for_dataset  # noqa: F401
