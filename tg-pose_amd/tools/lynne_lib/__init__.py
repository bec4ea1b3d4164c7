"""the reference's ``tools/lynne_lib`` names"""
