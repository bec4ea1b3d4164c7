"""``core.utils`` of the reference: farthest point sampling (farthest_points_torch)."""
