"""Box coder objects configs pass to the head (reference det3d/core/bbox/box_coders.py:40-109,
det3d/builder.py:399-432).  Decoding itself happens inside the head's device kernel; the
object carries the settings the reference's ``MultiGroupHead`` reads (``code_size``, ``n_dim``).
``encode`` / ``encode_torch`` are the host forms of what the target-assignment kernel computes for foreground anchors.
The device decoder takes ``n_dim`` 7 or 9 with either angle code; ``linear_dim`` and ``norm_velo`` are kept
but, as in the reference's ``decode_torch`` (which hands ``linear_dim`` to ``bin_loss`` and drops
``norm_velo``), never change the decode."""


class GroundBox3dCoderTorch:
    def __init__(self, linear_dim=False, vec_encode=False, n_dim=7, norm_velo=False):
        self.linear_dim = linear_dim
        self.vec_encode = vec_encode
        self.norm_velo = norm_velo
        self.n_dim = n_dim

    @property
    def code_size(self):
        return self.n_dim + 1 if self.vec_encode else self.n_dim

    def encode(self, boxes, anchors):
        """box_coders.py:46-53 (numpy): ``second_box_encode`` with this coder's settings."""
        from ..ops.box_np_ops import second_box_encode
        return second_box_encode(boxes, anchors, encode_angle_to_vector=self.vec_encode, smooth_dim=self.linear_dim,
                                 norm_velo=self.norm_velo)

    def encode_torch(self, boxes, anchors):
        """box_coders.py:101-104 over box_torch_ops.second_box_encode (:77-125); like it, ``norm_velo`` is not handed on."""
        import torch
        a, g = torch.split(anchors, 1, dim=-1), torch.split(boxes, 1, dim=-1)
        diagonal = torch.sqrt(a[4] ** 2 + a[3] ** 2)
        ret = [(g[0] - a[0]) / diagonal, (g[1] - a[1]) / diagonal, (g[2] - a[2]) / a[5]]
        if self.linear_dim:
            ret += [g[3] / a[3] - 1, g[4] / a[4] - 1, g[5] / a[5] - 1]
        else:
            ret += [torch.log(g[3] / a[3]), torch.log(g[4] / a[4]), torch.log(g[5] / a[5])]
        if anchors.shape[-1] > 7:
            ret += [g[6] - a[6], g[7] - a[7]]
        if self.vec_encode:
            ret += [torch.cos(g[-1]) - torch.cos(a[-1]), torch.sin(g[-1]) - torch.sin(a[-1])]
        else:
            ret.append(g[-1] - a[-1])
        return torch.cat(ret, dim=-1)


def build_box_coder(cfg):
    if cfg["type"] != "ground_box3d_coder":
        raise ValueError("unknown box_coder type")
    return GroundBox3dCoderTorch(cfg["linear_dim"], cfg["encode_angle_vector"],
                                 n_dim=cfg.get("n_dim", 9), norm_velo=cfg.get("norm_velo", False))
