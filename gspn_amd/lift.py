"""Predictions on a scan's own vertices: the prediction export stage of predict.py with a vertex of the scan's mesh in the
place of a scene point, for one scan at a time -- what the ScanNet instance benchmark wants, one mask value per vertex of
<scan>_vh_clean_2.ply.

The network's scene is a subset of the scan's vertices in the scan's own coordinates (data_prep.py:76-91 and dataset.py:89-105 pick points,
nothing re-centres or scales them), so the reference's rules for a scene point (test.py:163-205) apply to a vertex as they stand: the
nearest crop point of a detection behind the box test, the nearest seed, the sums, the order, the threshold.  One rule is new: a vertex
takes the semantic softmax row of the scene point nearest to it (src), the first minimum of the unfused fp32 (dx*dx + dy*dy) + dz*dz.
When the vertices are the scene's own, pairwise distinct points, src is the identity and scan_predictions reproduces scene_predictions.

vertex_tables is the nearest scene point and the nearest seed of every vertex -- nearest_point (nearest.py) for a known
set of more than NEAREST_FROM_M points, the first column of three_nn below; the two agree bit for bit --; gspn_lift_masks (csrc/lift.hip) fuses
nearest_in_sets and scene_confidence and never writes the (R, V) index tensor; gspn_scene_rank orders the rows as it does for a scene.
V differs from scan to scan, so nothing here is meant for a captured step.  No CPU fallback."""
import torch

from . import _lib as L
from ._args import _hole_parameters, _on_device, _parameters, _typed
from .components import COMPONENTS_MAX_F, component_filter
from .holes import hole_fill
from .mask_nms import mask_nms
from .nearest import nearest_point
from .predict import SCANNET_LABEL_MAP, SCENE_RANK_MAX_R, scene_rank
from .segments import SEGMENT_MAX_COUNTERS, SEGMENT_MAX_S, segment_label_vote, segment_vote
from .tf_interpolate import three_nn

__all__ = ["LIFT_MAX_P", "LIFT_MAX_V", "NEAREST_FROM_M", "lift_tile", "vertex_tables", "lift_masks", "scan_predictions"]

LIFT_MAX_P = 4096             # GSPN_LIFT_MAX_P of include/gspn_hip.h: a detection's crop points sit in LDS
LIFT_MAX_V = 1 << 24          # GSPN_LIFT_MAX_V
LIFT_MAX_R = 65535            # the detections are the grid's second dimension
NEAREST_FROM_M = 1024         # vertex_tables: a known set of more points than this goes to nearest_point; at or below it three_nn's one-wave
                              # kernel is the faster form up to 150 000 vertices (measured: DESIGN.md 4.22, profiles/nearest_stage.txt)
_SEARCHES = (None, "three_nn", "nearest_point")


def lift_tile(r, v):
    """the vertices one workgroup of gspn_lift_masks takes at (r, v): 1024 once that still gives every CU two workgroups, 256 below"""
    return 1024 if int(r) * ((int(v) + 1023) // 1024) >= 512 else 256


def _nearest_index(verts, known, search):
    """(V, 3) against (M, 3), both on the device -> (V,) int32: the first minimum, by the search that `search` names or the size picks"""
    if search == "nearest_point" or (search is None and known.shape[0] > NEAREST_FROM_M):
        return nearest_point(verts.unsqueeze(0), known.unsqueeze(0))[1][0]
    return three_nn(verts.unsqueeze(0), known.unsqueeze(0))[1][0, :, 0].contiguous()


def vertex_tables(verts, pc, pc_seed, fb_prob, search=None):
    """One scan.  verts (V, 3), pc (N, 3), pc_seed (S, 3), fb_prob (S, 2) float32 -> src (V,) int32: the scene point nearest to each vertex,
    vert_fb (V,) float32: fb_prob[nearest seed, 1] (inference._point_probabilities' rule on the vertex itself).  Both are the first
    column of three_nn: the first minimum of the unfused fp32 (dx*dx + dy*dy) + dz*dz, the lowest index among equal distances.
    search: None -- nearest_point for a known set of more than NEAREST_FROM_M points, three_nn below --, or "three_nn" / "nearest_point"
    to send both searches one way (the same bits either way; for comparing and measuring the two)."""
    verts = _typed(verts, torch.float32, 2, "verts")
    pc = _typed(pc, torch.float32, 2, "pc")
    pc_seed = _typed(pc_seed, torch.float32, 2, "pc_seed")
    fb_prob = _typed(fb_prob, torch.float32, 2, "fb_prob")
    if verts.shape[1] != 3 or pc.shape[1] != 3 or pc_seed.shape[1] != 3 or tuple(fb_prob.shape) != (pc_seed.shape[0], 2):
        raise ValueError("vertex_tables: expected verts (V, 3), pc (N, 3), pc_seed (S, 3) and fb_prob (S, 2), got %s, %s, %s and %s"
                         % (tuple(verts.shape), tuple(pc.shape), tuple(pc_seed.shape), tuple(fb_prob.shape)))
    if search not in _SEARCHES:
        raise ValueError("vertex_tables: search must be one of %s, got %r" % (_SEARCHES, search))
    if min(verts.shape[0], pc.shape[0], pc_seed.shape[0]) <= 0:
        raise ValueError("vertex_tables: empty input, verts %s, pc %s, pc_seed %s" % (tuple(verts.shape), tuple(pc.shape), tuple(pc_seed.shape)))
    verts, pc, pc_seed, fb_prob = _on_device(verts=verts, pc=pc, pc_seed=pc_seed, fb_prob=fb_prob)
    with torch.no_grad():
        src = _nearest_index(verts, pc, search)
        seed = _nearest_index(verts, pc_seed, search).long()
        return src, fb_prob[:, 1][seed].contiguous()


def lift_masks(verts, crops, boxes, masks, class_ids, src, sem_prob, vert_fb, mask_th=0.4, part=None):
    """gspn_lift_masks for one scan.  verts (V, 3), crops (R, P, 3), boxes (R, 6), masks (R, P) float32; class_ids (R,) int32; src (V,)
    int32; sem_prob (N, C), vert_fb (V,) float32; mask_th a Python float (a double); part: a float64 device tensor of at least
    gspn_lift_part_doubles(R, V) elements to use as the workspace (it need not be initialised), or None
    -> sem_conf, fb_conf (R,) float64, mask (R, V) uint8, mask_points (R,) int32.  With g = the mask value at the crop point nearest to the
    vertex inside the detection's box and 0 outside: sem_conf = sum(g * sem_prob[src, class]) / (1e-8 + sum(g)), fb_conf the same with
    vert_fb, every term exact in double, added in an order that depends on (R, V) alone; mask = float64(g) > mask_th.  A row whose class
    is outside [1, C) gets zeros everywhere; a src value outside [0, N) is clamped.  Raises NotImplementedError for P > 4096, R > 65535
    or V > 2^24, before anything has run."""
    verts = _typed(verts, torch.float32, 2, "verts")
    crops = _typed(crops, torch.float32, 3, "crops")
    boxes = _typed(boxes, torch.float32, 2, "boxes")
    masks = _typed(masks, torch.float32, 2, "masks")
    class_ids = _typed(class_ids, torch.int32, 1, "class_ids")
    src = _typed(src, torch.int32, 1, "src")
    sem_prob = _typed(sem_prob, torch.float32, 2, "sem_prob")
    vert_fb = _typed(vert_fb, torch.float32, 1, "vert_fb")
    v, (r, p), (n, c) = verts.shape[0], masks.shape, sem_prob.shape
    if (verts.shape[1] != 3 or tuple(crops.shape) != (r, p, 3) or tuple(boxes.shape) != (r, 6) or tuple(class_ids.shape) != (r,)
            or tuple(src.shape) != (v,) or tuple(vert_fb.shape) != (v,)):
        raise ValueError("lift_masks: expected verts (V, 3), crops (R, P, 3), boxes (R, 6), masks (R, P), class_ids (R,), src (V,), sem_prob (N, C) "
                         "and vert_fb (V,), got %s, %s, %s, %s, %s, %s, %s and %s"
                         % tuple(tuple(t.shape) for t in (verts, crops, boxes, masks, class_ids, src, sem_prob, vert_fb)))
    if min(v, r, p, n, c) <= 0:
        raise ValueError("lift_masks: empty input, verts %s, masks %s, sem_prob %s" % (tuple(verts.shape), tuple(masks.shape), tuple(sem_prob.shape)))
    mask_th = float(mask_th)
    if mask_th != mask_th:
        raise ValueError("lift_masks: mask_th is NaN")
    if p > LIFT_MAX_P or r > LIFT_MAX_R or v > LIFT_MAX_V:
        raise NotImplementedError("lift_masks: P <= %d, R <= %d and V <= %d (got %d, %d and %d)" % (LIFT_MAX_P, LIFT_MAX_R, LIFT_MAX_V, p, r, v))
    if part is not None:
        part = _typed(part, torch.float64, 1, "part")
    verts, crops, boxes, masks, class_ids, src, sem_prob, vert_fb = _on_device(
        verts=verts, crops=crops, boxes=boxes, masks=masks, class_ids=class_ids, src=src, sem_prob=sem_prob, vert_fb=vert_fb)
    dev = verts.device
    need = int(L.lib().gspn_lift_part_doubles(r, v))
    if part is None:
        part = torch.empty((need,), dtype=torch.float64, device=dev)
    elif part.numel() < need or not part.is_contiguous() or part.device != dev:
        raise ValueError("lift_masks: part must be a contiguous float64 tensor of at least %d elements on %s" % (need, dev))
    sem_conf = torch.empty((r,), dtype=torch.float64, device=dev)
    fb_conf = torch.empty((r,), dtype=torch.float64, device=dev)
    mask = torch.empty((r, v), dtype=torch.uint8, device=dev)
    mask_points = torch.empty((r,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().gspn_lift_masks(r, v, p, n, c, L.ptr(verts), L.ptr(crops), L.ptr(boxes), L.ptr(masks), L.ptr(class_ids), L.ptr(src),
                                        L.ptr(sem_prob), L.ptr(vert_fb), mask_th, L.ptr(part), L.ptr(sem_conf), L.ptr(fb_conf), L.ptr(mask),
                                        L.ptr(mask_points), L.stream()), "lift_masks")
    return sem_conf, fb_conf, mask, mask_points


_KEYS = ("detections", "rpointnet_mask_selected", "pc_coord_cropped_final_unnormalized", "pc_seed", "fb_prob", "sem_class_logits")


def scan_predictions(end_points, scene, verts, *, pc=None, sem_conf_th=0.01, fb_conf_th=0.01, mask_th=0.4, label_map=SCANNET_LABEL_MAP,
                     segments=None, num_segments=None, vote_th=0.5, mask_nms_th=None, faces=None, min_component=None, min_component_share=0.0,
                     max_hole=None, max_hole_share=1.0):
    """test.py:155-205 on the vertices of one scan.  end_points: rpointnet_inference's of a batch, as they are (read: detections (B, R, 8),
    rpointnet_mask_selected (B, R, P), pc_coord_cropped_final_unnormalized (B, R, P, 3), pc_seed, fb_prob, sem_class_logits (B, N, C));
    scene: the scan's slot in that batch; verts (V, 3) float32: the scan's vertices, in the coordinates of the scene's points; pc (B, N, 3):
    the batch the network ran on (end_points['pc'] when it is not passed); label_map: C integers.
    -> scene_predictions' dict with a leading dimension of 1 and V in the place of N -- order, label_ids, confidence, sem_conf, fb_conf,
    score, mask_points (1, R), count (1,), masks (1, R, V) uint8, every per-detection entry in output order; write_predictions(out_dir,
    scan, pred, 0) takes it as it is -- and 'src' (V,) int32, the scene point nearest to each vertex, for lifting anything else that is
    defined on the scene's points (semantic IoU on vertices: semantic_iou_counts(sem_class_logits[scene][src], vertex_seg_label)).
    segments (V,) int32 with num_segments: the compact segment ids of the vertices (segments.compact_segments), a value outside
    [0, num_segments) unsegmented.  Then every mask row is snapped to the segments by segments.segment_vote at vote_th
    before the rows are put in output order -- masks and mask_points change, the confidences, the order, the score and the count come
    from the soft values as before --, and the dict gains 'sem_label' (V,) int32: segment_label_vote of the first maximal column of
    sem_class_logits[scene][src].  Without segments the dict has exactly the keys and bits it had.
    mask_nms_th: a float in [0, 1), or None.  Then mask_nms.mask_nms at that IoU runs on the rows already in output order
    -- after the segment vote, where there is one --, with count and label_ids as they are (per class, like refine_detections): a row
    that an earlier kept row of its label overlaps above the threshold comes out all zero with mask_points 0, and the dict gains 'keep'
    (1, R) uint8; the confidences, the order, the score and the count are not touched.  With None the keys and bits are what they were.
    faces (F, 3) int32 with min_component: the scan's triangles (components.mesh_faces) and an int >= 1.  Then
    components.component_filter(min_vertices=min_component, min_share=min_component_share) runs in place on the hard rows behind the
    segment vote, BEFORE the rows are put in output order and before mask NMS, which must see the cleaned rows: a component of a row
    smaller than min_component vertices, or than min_component_share of the row's largest, is dropped.  masks and mask_points change and
    the dict gains 'components' and 'components_kept' (1, R) int32 in output order; the confidences, the order, the score and the count
    come from the soft values as before.  With neither faces nor a stage that needs them the keys and bits are what they were.
    faces with max_hole: an int >= 0.  Then holes.hole_fill(max_vertices=max_hole, max_share=max_hole_share) runs in place
    on the hard rows on the scan's own vertices `verts`, BEHIND the component filter where there is one, before the rows are put in
    output order and before mask NMS: a gap of at most max_hole vertices, and at most max_hole_share of the row's set vertices, that the
    row encloses on the mesh is filled.  masks and mask_points change and the dict gains 'holes' and 'holes_filled' (1, R) int32 in
    output order; the confidences, the order, the score and the count come from the soft values as before.  faces goes with at least one
    of min_component and max_hole, and each of the two needs faces: anything else raises ValueError.
    Raises ValueError on a missing key or a shape or dtype that does not fit, NotImplementedError for R > 1024, P > 4096 or V > 2^24,
    before anything runs."""
    for k in _KEYS:
        if k not in end_points:
            raise ValueError("scan_predictions: end_points has no %r (pass rpointnet_inference's end_points)" % k)
    if pc is None:
        if "pc" not in end_points:
            raise ValueError("scan_predictions: pass pc, the batch the network ran on (end_points has no 'pc')")
        pc = end_points["pc"]
    verts = _typed(verts, torch.float32, 2, "verts")
    pc = _typed(pc, torch.float32, 3, "pc")
    detections = _typed(end_points["detections"], torch.float32, 3, "detections")
    masks = _typed(end_points["rpointnet_mask_selected"], torch.float32, 3, "rpointnet_mask_selected")
    crops = _typed(end_points["pc_coord_cropped_final_unnormalized"], torch.float32, 4, "pc_coord_cropped_final_unnormalized")
    logits = _typed(end_points["sem_class_logits"], torch.float32, 3, "sem_class_logits")
    pc_seed = _typed(end_points["pc_seed"], torch.float32, 3, "pc_seed")
    fb_prob = _typed(end_points["fb_prob"], torch.float32, 3, "fb_prob")
    b, n, _ = pc.shape
    r, p = masks.shape[1:]
    c = logits.shape[2]
    v = verts.shape[0]
    if (verts.shape[1] != 3 or pc.shape[2] != 3 or tuple(detections.shape) != (b, r, 8) or masks.shape[0] != b or tuple(crops.shape) != (b, r, p, 3)
            or tuple(logits.shape[:2]) != (b, n) or pc_seed.shape[0] != b or pc_seed.shape[2] != 3
            or tuple(fb_prob.shape) != (b, pc_seed.shape[1], 2)):
        raise ValueError("scan_predictions: expected verts (V, 3), pc (B, N, 3), detections (B, R, 8), rpointnet_mask_selected (B, R, P), "
                         "pc_coord_cropped_final_unnormalized (B, R, P, 3), sem_class_logits (B, N, C), pc_seed (B, S, 3) and fb_prob (B, S, 2), "
                         "got %s, %s, %s, %s, %s, %s, %s and %s"
                         % tuple(tuple(t.shape) for t in (verts, pc, detections, masks, crops, logits, pc_seed, fb_prob)))
    if min(v, b, n, r, p, c, pc_seed.shape[1]) <= 0:
        raise ValueError("scan_predictions: empty input, verts %s, pc %s, rpointnet_mask_selected %s" % (tuple(verts.shape), tuple(pc.shape), tuple(masks.shape)))
    s = int(scene)
    if not 0 <= s < b:
        raise ValueError("scan_predictions: scene must lie in [0, %d), got %d" % (b, s))
    if isinstance(label_map, torch.Tensor):
        label_map = _typed(label_map, torch.int32, 1, "label_map")
    if len(label_map) != c:
        raise ValueError("scan_predictions: label_map must have one entry per class, %d, got %d" % (c, len(label_map)))
    thresholds = [float(t) for t in (sem_conf_th, fb_conf_th, mask_th)]
    if any(t != t for t in thresholds):
        raise ValueError("scan_predictions: a threshold is NaN")
    if segments is None:
        if num_segments is not None:
            raise ValueError("scan_predictions: num_segments without segments")
    else:
        segments = _typed(segments, torch.int32, 1, "segments")
        if tuple(segments.shape) != (v,):
            raise ValueError("scan_predictions: segments must name the segment of each of the %d vertices, got %s" % (v, tuple(segments.shape)))
        if num_segments is None or int(num_segments) < 0:
            raise ValueError("scan_predictions: segments needs num_segments >= 0 (segments.compact_segments gives both), got %r" % (num_segments,))
        num_segments, vote_th = int(num_segments), float(vote_th)
        if not 0.0 <= vote_th < 1.0:
            raise ValueError("scan_predictions: vote_th must lie in [0, 1), got %r" % vote_th)
    if mask_nms_th is not None:
        mask_nms_th = float(mask_nms_th)
        if not 0.0 <= mask_nms_th < 1.0:
            raise ValueError("scan_predictions: mask_nms_th must lie in [0, 1), got %r" % mask_nms_th)
    if (faces is None and min_component is not None) or (faces is not None and min_component is None and max_hole is None):
        raise ValueError("scan_predictions: faces and min_component go together (got faces %s, min_component %r)"
                         % ("None" if faces is None else "given", min_component))
    if faces is None and max_hole is not None:
        raise ValueError("scan_predictions: faces and max_hole go together (got faces None, max_hole %r)" % (max_hole,))
    if faces is not None:
        faces = _typed(faces, torch.int32, 2, "faces")
        if faces.shape[1] != 3:
            raise ValueError("scan_predictions: faces must be (F, 3) (components.mesh_faces), got %s" % (tuple(faces.shape),))
        if min_component is not None:
            min_component, min_component_share = _parameters(min_component, min_component_share, "scan_predictions")
        if max_hole is not None:
            max_hole, max_hole_share = _hole_parameters(max_hole, max_hole_share, "scan_predictions")
    if r > SCENE_RANK_MAX_R or p > LIFT_MAX_P or v > LIFT_MAX_V:
        raise NotImplementedError("scan_predictions: R <= %d, P <= %d and V <= %d (got %d, %d and %d)"
                                  % (SCENE_RANK_MAX_R, LIFT_MAX_P, LIFT_MAX_V, r, p, v))
    if segments is not None:
        if num_segments > SEGMENT_MAX_S or (r + 1) * num_segments > SEGMENT_MAX_COUNTERS or num_segments * c > SEGMENT_MAX_COUNTERS:
            raise NotImplementedError("scan_predictions: num_segments <= %d, (R + 1) * num_segments and num_segments * C <= %d (got %d)"
                                      % (SEGMENT_MAX_S, SEGMENT_MAX_COUNTERS, num_segments))
        segments, = _on_device(segments=segments)
    if faces is not None:
        if faces.shape[0] > COMPONENTS_MAX_F:
            raise NotImplementedError("scan_predictions: F <= %d (got %d)" % (COMPONENTS_MAX_F, faces.shape[0]))
        faces, = _on_device(faces=faces)
    verts, pc, detections, masks, crops, logits, pc_seed, fb_prob = _on_device(
        verts=verts, pc=pc, detections=detections, rpointnet_mask_selected=masks, pc_coord_cropped_final_unnormalized=crops,
        sem_class_logits=logits, pc_seed=pc_seed, fb_prob=fb_prob)
    with torch.no_grad():
        det = detections[s]
        src, vert_fb = vertex_tables(verts, pc[s], pc_seed[s], fb_prob[s])
        sem_prob = torch.softmax(logits[s:s + 1], -1)[0]                                                # inference._point_probabilities' table of the scene
        class_ids = det[:, 6].int()                                                                     # :180, .astype(np.int32)
        sem_conf, fb_conf, mask, mask_points = lift_masks(verts, crops[s], det[:, :6], masks[s], class_ids, src, sem_prob, vert_fb, thresholds[2])
        sem_label = None
        if segments is not None:                                                                        # 4.23: in place, the hard masks alone
            mask, mask_points = segment_vote(mask, segments, num_segments, vote_th, out=mask)
            own = logits[s].max(-1).indices.int().index_select(0, src.long())                           # the first maximal column, as gspn_sem_iou_counts takes it
            sem_label = segment_label_vote(own, segments, num_segments, c)
        components = None
        if min_component is not None:                                                                   # 4.25: in place, behind the vote, before the order
            mask, mask_points, components, kept = component_filter(mask, faces, min_vertices=min_component, min_share=min_component_share, out=mask)
        holes = None
        if max_hole is not None:                                                                        # 4.26: in place, behind the filter, before the order
            mask, mask_points, holes, holes_filled = hole_fill(mask, faces, verts, max_vertices=max_hole, max_share=max_hole_share, out=mask)
        order, count, label_ids, confidence, score = scene_rank(det[None, :, 7], class_ids[None], sem_conf[None], fb_conf[None], thresholds[0],
                                                                thresholds[1], label_map)
        at = order[0].long()
        pred = {
            "order": order, "count": count, "label_ids": label_ids, "confidence": confidence,
            "sem_conf": sem_conf[at][None], "fb_conf": fb_conf[at][None], "score": score,
            "masks": mask.index_select(0, at)[None], "mask_points": mask_points[at][None], "src": src,
        }
        if sem_label is not None:
            pred["sem_label"] = sem_label
        if components is not None:
            pred["components"], pred["components_kept"] = components[at][None], kept[at][None]
        if holes is not None:
            pred["holes"], pred["holes_filled"] = holes[at][None], holes_filled[at][None]
        if mask_nms_th is not None:                                                                     # 4.24: in place, on the rows in output order
            pred["masks"], pred["keep"], pred["mask_points"] = mask_nms(pred["masks"], count, label_ids, iou_th=mask_nms_th, out=pred["masks"])
        return pred
