"""The patch bay (include/dspi.h: dspi_process_patched, dspi_patched_bytes) as a model in plain Python, written from the header's prose: where
every stream's run starts in `in`, which launch serves which stream, and the column a patch into a tiled view resolves to.  What
dspi_amd/csrc/dspi_patch.cpp (the layout and the plan) is held to through tests/patch_driver.cpp, and — with tests/linkrx_model.py and
tests/spdifrx_model.py for the words — what dspi_process_patched is held to on the GPU."""
import numpy as np

import linkrx_model as LM
import spdifrx_model as M

PCM16, PCM24, SPDIF, LINK = 16, 24, 1, 2
SIZE = {PCM16: 4, PCM24: 6, SPDIF: 16, LINK: 0}      # bytes per frame of `in`
PATCH = np.dtype([("view", "<u4"), ("line", "<u4"), ("kind", "<u4")])
MAX_VIEWS = 8


def offsets(sources, F: int):
    """offset[s] = offset[s - 1] + F * size[s - 1], rounded up to 16 when sources[s] is S/PDIF; a LINK stream occupies zero bytes -> n + 1 values"""
    at, out = 0, []
    for src in sources:
        if src == SPDIF: at = (at + 15) // 16 * 16
        out.append(at)
        at += F * SIZE[int(src)]
    return out + [at]


def server(s: int, sources, active, views, patches):
    """which launch serves stream s: None (paused), "intake", "receiver" (the S/PDIF runs of `in`), ("spdifrx", v) / ("i2s", v) (the lines of the
    stream-major view v), or "patchrx" (every tiled view's patches together)"""
    if not active[s]: return None
    src = int(sources[s])
    if src in (PCM16, PCM24): return "intake"
    if src == SPDIF: return "receiver"
    v, kind = int(patches[s]["view"]), int(patches[s]["kind"])
    if int(views[v]["tile_streams"]): return "patchrx"
    return ("spdifrx" if kind == LM.SPDIF else "i2s", v)


def column(view, line: int) -> int:
    """the address of the first word of the column of `line` in its region of a TILED view: the region starts at word ((s / R * P + p) * F) * 4 * R,
    the column is c = s % R"""
    P, R, F = int(view["n_pairs"]), int(view["tile_streams"]), int(view["n_frames"])
    s, p = divmod(line, P)
    return int(view["wire"]) + 4 * (((s // R * P + p) * F) * 4 * R + s % R)


def plan(sources, active, views, patches, F: int) -> dict:
    """everything tests/patch_driver.cpp prints for a valid case, as the strings it prints"""
    n = len(sources)
    who = [server(s, sources, active, views, patches) for s in range(n)]
    out = {}
    out["flags"] = [int("intake" in who), int("receiver" in who), int("patchrx" in who), int(any(w == "patchrx" and patches[s]["kind"] == LM.SPDIF for s, w in enumerate(who)))]
    out["in_offsets"] = offsets(sources, F)
    out["in_kinds"] = [int(sources[s]) if who[s] in ("intake", "receiver") else 0 for s in range(n)]
    out["pcm_mask"] = [int(w == "intake") for w in who]
    out["views"] = []
    for v, view in enumerate(views):
        mine = [s for s in range(n) if active[s] and sources[s] == LINK and patches[s]["view"] == v]
        tiled = bool(int(view["tile_streams"]))
        d = dict(used=int(bool(mine)), any_spdif=int(any(who[s] == ("spdifrx", v) for s in mine)), any_i2s=int(any(who[s] == ("i2s", v) for s in mine)))
        if mine and not tiled:
            served = {s for s in mine}
            d["offsets"] = [int(patches[s]["line"]) * F * 4 * 4 if s in served else 0 for s in range(n)] + [0]      # (the region starts at word (L * F) * 4)
            d["links"] = [f'{int(patches[s]["line"])}:{int(patches[s]["kind"])}' if s in served else "0:0" for s in range(n)]
            d["kinds"] = [int(patches[s]["kind"]) if s in served else 0 for s in range(n)]
        out["views"].append(d)
    if "patchrx" in who:
        out["cols"] = [f'{column(views[int(patches[s]["view"])], int(patches[s]["line"]))}:{int(views[int(patches[s]["view"])]["tile_streams"])}:{int(patches[s]["kind"])}' if w == "patchrx" else "0:0:0"
                       for s, w in enumerate(who)]
    return out


def fed(s: int, wires, views, patches, rx: dict | None) -> np.ndarray:
    """what a LINK stream is fed: the model's decode of its line where it lies (wires[v]: the flat uint32 buffer of view v) -> pairs int32 [F][2]"""
    v = int(patches[s]["view"])
    view = views[v]
    return LM.decode(wires[v], int(view["n_pairs"]), int(view["tile_streams"]), int(view["n_frames"]), int(patches[s]["line"]), int(patches[s]["kind"]), rx)


def needs_rx(sources, active, patches) -> bool:
    return any(active[s] and (sources[s] == SPDIF or (sources[s] == LINK and patches[s]["kind"] == LM.SPDIF)) for s in range(len(sources)))
