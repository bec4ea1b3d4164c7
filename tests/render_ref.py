"""NumPy restatement of the depth renderer's contract (DESIGN.md section 3 "The depth renderer"; the kernel is csrc/render.hip).
Written from the contract's text, not from the kernel: fp32 products and sums that each round on their own, correctly rounded
fp32 division, int64 edge functions, int64 -> fp32 round-to-nearest.  One Python step per triangle whose pixel box is not empty,
vectorised over that box."""
import numpy as np

F = np.float32
GUARD = 1 << 22


def project(verts, pose, camk, near):
    """verts (V,3), pose (3,4) = [s R | t], camk (fx, fy, cx, cy) -> X, Y int64 (1/256 px), iz fp32, flag (0 ok, 1 near, 2 guard)"""
    v = np.asarray(verts, dtype=F)
    m = np.asarray(pose, dtype=F).reshape(3, 4)
    fx, fy, cx, cy = (F(k) for k in camk)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    p = [((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)]
    ok = p[2] > F(near)                                          # False for a NaN
    pz = np.where(ok, p[2], F(1))
    with np.errstate(all="ignore"):
        u = (fx * (p[0] / pz) + cx) * F(256)
        w = (fy * (p[1] / pz) + cy) * F(256)
        inside = (np.abs(u) <= F(GUARD)) & (np.abs(w) <= F(GUARD))   # False for a NaN
        good = ok & inside
        X = np.where(good, np.rint(np.where(good, u, 0)), 0).astype(np.int64)
        Y = np.where(good, np.rint(np.where(good, w, 0)), 0).astype(np.int64)
        iz = F(1) / pz
    flag = np.where(ok, np.where(inside, 0, 2), 1)
    return X, Y, iz.astype(F), flag


def _orient(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def render_scene(meshes, instances, camk, H, W, near=0.01):
    """meshes: list of (verts (V,3) float32, faces (F,3) int); instances: list of (mesh index, inst_id, pose (3,4)) in slot order.
    -> dict z (H,W) float32 (+inf empty), face (H,W) int32 (-1), mask uint8, depth uint16, slot (H,W) int32 (-1), visible (n,),
    bbox (n,4) (y1,x1,y2,x2), dropped (2,)"""
    zbuf = np.full((H, W), np.inf, dtype=F)
    slotbuf = np.full((H, W), 1 << 30, dtype=np.int64)
    facebuf = np.full((H, W), 1 << 30, dtype=np.int64)
    dropped = np.zeros(2, dtype=np.int32)
    for slot, (mi, _, pose) in enumerate(instances):
        verts, faces = meshes[mi]
        faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
        X, Y, iz, flag = project(verts, pose, camk, near)
        fl = flag[faces]                                                          # (F,3)
        is_near = (fl == 1).any(1)
        is_guard = ~is_near & (fl == 2).any(1)
        dropped += np.array([is_near.sum(), is_guard.sum()], dtype=np.int32)
        x = X[faces]
        y = Y[faces]
        area = _orient(x[:, 0], y[:, 0], x[:, 1], y[:, 1], x[:, 2], y[:, 2])
        x0 = np.maximum(-((-x.min(1)) // 256), 0)                                 # the first sample at or after the least coordinate
        x1 = np.minimum(x.max(1) // 256, W - 1)
        y0 = np.maximum(-((-y.min(1)) // 256), 0)
        y1 = np.minimum(y.max(1) // 256, H - 1)
        live = ~is_near & ~is_guard & (area != 0) & (x0 <= x1) & (y0 <= y1)
        for t in np.nonzero(live)[0]:
            order = (0, 1, 2) if area[t] > 0 else (0, 2, 1)                       # oriented: the doubled area is positive
            vx, vy, viz = x[t, order], y[t, order], iz[faces[t, order]]
            A = abs(int(area[t]))
            px = (np.arange(x0[t], x1[t] + 1, dtype=np.int64) * 256)[None, :]
            py = (np.arange(y0[t], y1[t] + 1, dtype=np.int64) * 256)[:, None]
            inside = True
            w = []
            for k in range(3):                                                    # edge k is opposite vertex k
                a, b = (k + 1) % 3, (k + 2) % 3
                dx, dy = vx[b] - vx[a], vy[b] - vy[a]
                E = dx * (py - vy[a]) - dy * (px - vx[a])
                top_left = dy < 0 or (dy == 0 and dx > 0)
                inside = inside & ((E >= 0) if top_left else (E > 0))
                w.append(E.astype(F) / F(A))
            if not np.any(inside):
                continue
            with np.errstate(all="ignore"):
                invz = (w[0] * viz[0] + w[1] * viz[1]) + w[2] * viz[2]
                z = F(1) / invz
            sl = (slice(y0[t], y1[t] + 1), slice(x0[t], x1[t] + 1))
            zb, sb, fb = zbuf[sl], slotbuf[sl], facebuf[sl]
            wins = inside & ((z < zb) | ((z == zb) & ((slot < sb) | ((slot == sb) & (t < fb)))))
            zb[wins] = z[wins]
            sb[wins] = slot
            fb[wins] = t
    hit = slotbuf < (1 << 30)
    ids = np.array([i[1] for i in instances] + [0], dtype=np.uint8)
    mask = np.where(hit, ids[np.where(hit, slotbuf, len(instances))], 0).astype(np.uint8)
    with np.errstate(all="ignore"):
        mm = np.rint(zbuf * F(1000))
    depth = np.where(hit & (mm <= 65535), mm, 0).astype(np.uint16)
    n = len(instances)
    visible = np.zeros(n, dtype=np.int32)
    bbox = np.zeros((n, 4), dtype=np.int32)
    for s in range(n):
        ys, xs = np.nonzero(hit & (slotbuf == s))
        visible[s] = len(ys)
        if len(ys):
            bbox[s] = [ys.min(), xs.min(), ys.max() + 1, xs.max() + 1]
    return dict(z=zbuf, face=np.where(hit, facebuf, -1).astype(np.int32), slot=np.where(hit, slotbuf, -1).astype(np.int32), mask=mask,
                depth=depth, visible=visible, bbox=bbox, dropped=dropped)


def render(meshes, scene_ptr, inst_mesh, inst_id, inst_pose, camk, H, W, near=0.01):
    """the kernel's call: S scenes -> the outputs stacked as ops.render_depth returns them"""
    S = len(scene_ptr) - 1
    outs = []
    for s in range(S):
        r = range(int(scene_ptr[s]), int(scene_ptr[s + 1]))
        outs.append(render_scene(meshes, [(int(inst_mesh[i]), int(inst_id[i]), inst_pose[i]) for i in r], camk[s], H, W, near))
    cat = lambda k, shape, dt: (np.concatenate([o[k] for o in outs]) if outs else np.zeros(shape, dt))
    return dict(z=np.stack([o["z"] for o in outs]), face=np.stack([o["face"] for o in outs]), mask=np.stack([o["mask"] for o in outs]),
                depth=np.stack([o["depth"] for o in outs]), visible=cat("visible", (0,), np.int32), bbox=cat("bbox", (0, 4), np.int32),
                dropped=np.stack([o["dropped"] for o in outs]))


def pose34(R, t, s=1.0):
    """[s R | t] as the kernel reads it: float32 (3,4)"""
    return np.concatenate([np.asarray(R, dtype=np.float64) * float(s), np.asarray(t, dtype=np.float64).reshape(3, 1)], 1).astype(F)
