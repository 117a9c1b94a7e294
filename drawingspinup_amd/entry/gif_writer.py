"""`python gif_writer.py --data_dir D --uid U` (3_style_translator/gif_writer.py): one GIF per
action and stylisation result, `<uid>/mesh/gif/<action>_<result>.gif`, from the frames the test
stages wrote under `<uid>/mesh/blender_render/<action>/res_stage{1,2}_*`.  Stage-2 results are
used when the rest pose has any, stage-1 results otherwise; rest_pose itself is not animated."""
import argparse
import os

from PIL import Image


def run(argv=None):
    ap = argparse.ArgumentParser(description="generate GIF file")
    ap.add_argument("--data_dir", default="../dataset/AnimatedDrawings/preprocessed", help="data root")
    ap.add_argument("--uid", default="0dd66be9d0534b93a092d8c4c4dfd30a", help="image uid")
    args = ap.parse_args(argv)
    mesh_dir = os.path.join(args.data_dir, args.uid, "mesh")
    render_dir = os.path.join(mesh_dir, "blender_render")
    actions = sorted(d for d in os.listdir(render_dir) if not d.startswith(".") and d != "rest_pose")
    # the result folders are looked up under rest_pose, as the reference does; a tree rendered
    # with --test only has none, then the action's own folders decide
    def results(folder, stage):
        return sorted(d for d in os.listdir(folder) if d.startswith(f"res_stage{stage}_"))
    written = []
    for action in actions:
        probe = os.path.join(render_dir, "rest_pose")
        if not os.path.isdir(probe):
            probe = os.path.join(render_dir, action)
        kinds = results(probe, 2) or results(probe, 1)
        for kind in kinds:
            folder = os.path.join(render_dir, action, kind)
            if not os.path.isdir(folder):
                continue
            names = sorted(n for n in os.listdir(folder) if n.endswith(".png"))
            if not names:
                continue
            print(action, kind)
            frames = [Image.open(os.path.join(folder, n)) for n in names]
            os.makedirs(os.path.join(mesh_dir, "gif"), exist_ok=True)
            dst = os.path.join(mesh_dir, "gif", f"{action}_{kind}.gif")
            frames[0].save(dst, save_all=True, append_images=frames[1:], duration=30, disposal=2, loop=0)
            written.append(dst)
    return written


if __name__ == "__main__":
    run()
