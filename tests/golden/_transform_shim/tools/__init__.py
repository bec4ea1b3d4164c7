"""Stand-in for the reference's ``tools`` package while tests/golden/make_view_sampler_golden.py loads its
``tools/lynne_lib/view_sampler.py`` by path: that file does ``from tools import transform``, and the reference's tree holds no
``tools/transform.py``."""
