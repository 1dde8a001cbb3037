"""The reference's BVH loader (motion/bvh.py:22-138) restated for the tests: the text is split into lines, a line into whitespace-separated
words, and every number goes through Python's float().  Joints are numbered as their ROOT / JOINT lines appear; a joint's parent is the
joint whose block is open; an OFFSET inside an End Site block is dropped; the rotation order is read from the first CHANNELS line.  With
three channels per joint a frame is the root's position and then three angles per joint, every other joint's position being its offset;
with six channels per joint a frame is (position, angles) per joint.  Everything is float64, as the reference returns it.

``motion_tokens`` is the same split applied to a numeric block alone: the words, in order, and the float64 values."""
import numpy as np

CHANNEL_AXIS = {"Xrotation": "x", "Yrotation": "y", "Zrotation": "z"}


def load(text):
    if isinstance(text, bytes):
        text = text.decode()
    names, parents, offsets = [], [], []
    open_joint, in_end_site = -1, False
    order, channels, frames, frametime = None, None, None, None
    rows = []
    for line in text.splitlines():
        words = line.split()
        if not words or words[0] in ("HIERARCHY", "MOTION", "{"):
            continue
        if words[0] in ("ROOT", "JOINT"):
            names.append(words[1]); parents.append(open_joint); offsets.append([0.0, 0.0, 0.0])
            open_joint = len(names) - 1
        elif words[0] == "}":
            if in_end_site:
                in_end_site = False
            else:
                open_joint = parents[open_joint]
        elif words[0] == "OFFSET":
            if not in_end_site:
                offsets[open_joint] = [float(w) for w in words[1:4]]
        elif words[0] == "CHANNELS":
            channels = int(words[1])
            if order is None:
                order = "".join(CHANNEL_AXIS[w] for w in words[2 + channels - 3: 2 + channels])
        elif words[:2] == ["End", "Site"]:
            in_end_site = True
        elif words[0] == "Frames:":
            frames = int(words[1])
        elif words[:2] == ["Frame", "Time:"]:
            frametime = float(words[2])
        else:
            rows.append([float(w) for w in words])
    V = len(names)
    offsets = np.array(offsets, dtype=np.float64).reshape(V, 3)
    data = np.array(rows, dtype=np.float64)
    assert data.shape[0] == frames, (data.shape, frames)
    positions = np.repeat(offsets[None], frames, axis=0)
    if channels == 3:
        assert data.shape[1] == 3 + 3 * V
        positions[:, 0] = data[:, :3]
        rotations = data[:, 3:].reshape(frames, V, 3)
    else:
        assert channels == 6 and data.shape[1] == 6 * V
        data = data.reshape(frames, V, 6)
        positions, rotations = data[..., :3].copy(), data[..., 3:].copy()
    return {"rotations": rotations, "positions": positions, "offsets": offsets, "parents": np.array(parents), "names": names, "order": order,
            "frametime": frametime, "channels": channels}


def motion_tokens(block):
    if isinstance(block, bytes):
        block = block.decode()
    words = [w for line in block.splitlines() for w in line.split()]
    return words, np.array([float(w) for w in words], dtype=np.float64)
