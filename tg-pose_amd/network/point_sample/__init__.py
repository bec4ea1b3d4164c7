"""``network.point_sample`` of the reference: surface sampling of meshes (pc_sample_sphere)."""
