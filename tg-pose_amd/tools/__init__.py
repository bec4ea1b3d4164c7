"""The reference's ``tools`` helpers this repository rebuilds: the Ranger optimizer and the flat-and-anneal schedule
(``tools.torch_utils.solver``) and the two trainer builders of ``tools.training_utils``."""
