"""``tools.render`` of the reference: its renderer interface (renderer.py), with the HIP depth rasteriser as the back end."""
