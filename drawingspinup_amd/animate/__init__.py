"""Frame rendering between reconstruction and stylisation: `<uid>/mesh/*.obj` -> the colour /
position / edge frames of `<uid>/mesh/blender_render/<action>/` (3_style_translator/run_render.py +
blender_animation.py), for the two actions that need no rig:

    rest_pose      one frame of the rest mesh — the training input
    rest_rotate    a turntable of the rest mesh — the reference's fallback when a character has no
                   animation (run_render.py:81-82)

For those the reference's Blender is an orthographic rasteriser of a vertex-coloured mesh, run once
with the colours and once with the normalised positions (blender_animation.py:26-33,92-121);
pos2edge (run_render.py:31-57) runs on the position pass.  Both passes, all frames and the edges
run on the device (csrc/mesh_render.hip).  A caller-supplied (F,V,3) vertex animation is accepted
as well: a skinned animation made elsewhere renders through the same path.

Deviations from the reference (Blender itself is not here to compare against): by default a box
filter over ss^2 sub-samples stands in for Blender's pixel filter (`pixel_filter="eevee"` or
`"cycles"` puts a Blackman-Harris window in its place, see `pixel_filter`; the widths are read from
Blender's source and unpinned); no view transform or tone curve is applied (the reference selects
'Standard'); the turntable's frame count lives in a .blend file that is not in the snapshot, so it
is a parameter.

Textured frames: `read_obj_textured` keeps a textured export's uvs and atlas, and `render_frames` /
`animate_mesh` with `texture=` and `uvs=` sample the atlas inside the rasteriser's resolve, per
sub-sample (nearest, bilinear, or trilinear on the atlas's mip pyramid — `texture_filter="trilinear"`,
isotropic, for an atlas finer than the sample lattice —, or `texture_filter="anisotropic"` with up to
`max_anisotropy` probes of that pyramid along the long axis of each face's footprint, for the faces
that turn edge-on towards the silhouette; no seam blending),
where Blender reads `map_Kd`.
Without them the colour frames interpolate the vertex colours, as before.

Rigged animations: `read_bvh` reads a skeleton and a motion clip, `bone_heat_weights` binds the mesh
to the skeleton (distances, visibility and the solve on the device, csrc/mesh_skin.hip),
`animate_mesh` skins every frame on the device and renders it through the same rasteriser.  The
weighting follows the published bone-heat form, not Blender's source; the view box is taken over
the deformed vertices where Blender uses the object's bound_box; there is no automatic joint
placement (`fit_to_mesh` only scales and centres a skeleton); the 30 degree turn
that blender_animation.py:17-18 applies to two named clips is not restated.  FBX is not read.
A rig from marks (rig.py): `read_marks` reads the 2-D joint marks of a drawing (AnimatedDrawings'
char_cfg.yaml), `pixels_to_mesh` takes them to the exported OBJ's frame, `lift_marks` places every
joint at the middle of the mesh's thickness under its mark (one thickness map on the device,
csrc/mesh_thickness.hip), and `retarget_clip` turns any BVH clip into a clip of that skeleton by the
world directions of the source's bones, whatever pose the character was drawn in.
`animate_mesh(skinning="dual_quaternion")` blends unit dual quaternions instead of matrices (Blender's
"Preserve Volume"; `dual_quaternions` makes the table), and `resample_clip` brings a clip to another
frame rate (slerp of the local rotations).  `animate_mesh(corrective_iterations=N)` smooths the
skinned frames and puts the rest mesh's detail back (delta mush, Blender's Corrective Smooth;
`smoothing_topology` builds the welded graph it walks): it repairs creases from bad weights, not the
collapse of a twisted limb.  `animate_mesh(skinning="centre_of_rotation")` rotates every vertex about
its own centre of rotation (Le & Hodgins 2016; `cor_centres` computes them once per character, a sum
over all vertex-triangle pairs on the device): the radius is kept as with dual quaternions, without
their bulge on the outside of a sharp bend.
"""
from .render import (DEFAULT_SIZE, DEFAULT_SPAN, PIXEL_FILTER_PRESETS, frame_window, motion_frames, pixel_filter,
                     position_colours, read_obj, read_obj_textured, render_frames, rest_pose, rest_rotate)
from .skeleton import (Clip, Skeleton, dual_quaternions, fit_to_mesh, quaternion_rotations, read_bvh, resample_clip,
                       rest_clip, rotation_quaternions, skinning_matrices)
from . import corrective
from .corrective import smoothing_topology
from .skin import animate_mesh, bone_heat_weights, cor_centres
from . import rig
from .rig import lift_marks, minimal_rotation, pixels_to_mesh, read_marks, retarget_clip

__all__ = ["Clip", "Skeleton", "animate_mesh", "bone_heat_weights", "cor_centres", "dual_quaternions", "fit_to_mesh",
           "quaternion_rotations", "read_bvh", "resample_clip", "rest_clip", "rotation_quaternions", "skinning_matrices", "DEFAULT_SIZE", "DEFAULT_SPAN", "PIXEL_FILTER_PRESETS", "frame_window", "motion_frames", "pixel_filter", "position_colours",
           "read_obj", "read_obj_textured", "render_frames", "rest_pose", "rest_rotate", "smoothing_topology",
           "lift_marks", "minimal_rotation", "pixels_to_mesh", "read_marks", "retarget_clip"]
